#!/usr/bin/env python
"""Record tests/golden/fw_plan.npz: what the fused forward's host driver decides for every case of tests/test_fw_plan_host.py.

    python scripts/record_fw_plan.py [--lib PATH/libiwvi_hip.so] [--out tests/golden/fw_plan.npz]

Run it against a library whose answers are to be pinned, on a host WITHOUT a device: the real entries (``iwvi_dgp_forward``,
``iwvi_dgp_predict_density``, ``iwvi_dgp_predict_samples``) are called with made-up pointers.  There they plan the call, set the variant
word, and stop at ``hipFuncSetAttribute`` with ``IWVI_ERR_LAUNCH`` and the text "hipFuncSetAttribute(k_dgp_forward, N B): ..." -- N is the
plan's LDS bytes; a refusal returns its own status and text before that.  The launch grid is not observable this way; it is
``ceil(T / (16 * ns))`` with the recorded ``ns``, its definition.  With a device present the made-up pointers would reach a kernel: the
script refuses to start."""
import argparse
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def observe(lib, call):
    """(status, word, grid, lds, text): status 0 = planned (stopped at the first HIP call)."""
    c = call.c
    a = call.forward_args()
    if c["tail"] == 0:
        rc = lib.iwvi_dgp_forward(*a)
    elif c["tail"] == 1:
        rc = lib.iwvi_dgp_predict_density(a[0], a[1], a[2], a[3], a[6], a[7], call.row_mod, call.row_div, a[11], None, a[12], a[13], a[14], a[14], None)
    else:
        rc = lib.iwvi_dgp_predict_samples(a[0], a[1], a[2], a[3], a[7], call.row_mod, call.row_div, a[11], None, call.z_y, a[12], a[13], a[14], None)
    text = lib.iwvi_last_error().decode() if rc else ""
    m = re.match(r"hipFuncSetAttribute\(k_dgp_forward, (\d+) B\)", text)
    if rc == 0:                                       # an empty call
        return 0, 0, 0, 0, ""
    if not (rc == -2 and m):
        return rc, 0, 0, 0, text
    word = lib.iwvi_debug_last_forward_variant()
    nsamp = 16 * (word & 0xff)
    return 0, word, (call.T + nsamp - 1) // nsamp, int(m.group(1)), ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fw_plan.npz"))
    args = ap.parse_args()
    import torch
    if torch.cuda.device_count() > 0:
        sys.exit("record_fw_plan.py: a device is present; the made-up pointers must never meet one")
    from dgps_with_iwvi_amd import _abi
    import test_fw_plan_host as t
    lib = ctypes.CDLL(args.lib or _abi.LIB_PATH)
    for name in ("iwvi_dgp_forward", "iwvi_dgp_predict_density", "iwvi_dgp_predict_samples", "iwvi_debug_last_forward_variant",
                 "iwvi_last_error", "iwvi_debug_set_option"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _abi.PROTOTYPES[name]
    cases = t.grid()
    res = np.zeros((len(cases), 4), dtype=np.int64)
    err_case, err_text = [], []
    for opt, idx in t.each_option(cases):
        if opt:
            lib.iwvi_debug_set_option(opt[0].encode(), opt[1])
        for i in idx:
            r = observe(lib, t.Call(cases[i]))
            res[i] = r[:4]
            if r[0]:
                err_case.append(int(i))
                err_text.append(r[4])
        if opt:
            lib.iwvi_debug_set_option(opt[0].encode(), 0)
    order = np.argsort(err_case)
    copy2 = np.array(observe(lib, t.copy_list_call(2))[:4], dtype=np.int64)   # (three and four such layers overrun the old list: not run)
    np.savez_compressed(args.out, cases=cases, status=res[:, 0].astype(np.int8), word=res[:, 1].astype(np.int32), grid=res[:, 2], lds=res[:, 3],
                        err_case=np.array(err_case, dtype=np.int64)[order], err_text=np.array(err_text)[order], copy2=copy2)
    ok = res[:, 0] == 0
    rows = set(zip(cases[ok, 0].tolist(), res[ok, 1].tolist()))
    print("%d cases, %d refusals, %d (tail, word) rows, %d distinct words; not reached: %s; copy2 %s; %d bytes" % (
        len(cases), int((~ok).sum()), len(rows), len({w for _, w in rows}), sorted(t.expected_rows() - rows), copy2.tolist(), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
