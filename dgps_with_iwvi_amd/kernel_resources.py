"""Register / scratch budget of every kernel in libiwvi_hip.so, read from the code objects' metadata (no GPU needed).

The layer kernel's hot variants sit at the 256-VGPR limit: a source change anywhere in the layer loop can push one of them into
scratch, and a variant that only the large configs take then regresses unnoticed (round 4: the five-sub-tile large-M variant went
216 B into scratch, configs[3] 1.27 -> 1.43 ms, for four commits).  ``check()`` is run by ``__graft_entry__.build()`` and by
tests/test_kernel_resources.py: it fails when a ``k_dgp_forward`` or ``k_bw_chain`` instantiation (the predictive and sampling variants of the
forward included), ``k_sample_stats``, ``k_sample_scores``, ``k_energy_score``, ``k_psis_summary``, ``k_kde_grid`` or a likelihood-tail kernel (every ``k_lik_*``, ``k_mc_*``, ``k_xl_*``, ``k_bo_*``, ``k_hg_*``, the ``*_mix`` kernels of the predictive mixture and the sampling kernel ``k_lik_sample`` included) the SGHMC update ``k_sghmc_step``, a CVAE kernel (``k_cvae_*``) or a k-means kernel (``k_km_*``) uses scratch memory
(``.private_segment_fixed_size`` > 0) beyond what ``ALLOWED_SCRATCH`` lists, when a listed spill count grows, or when a kernel listed in ``MAX_VGPRS`` exceeds its VGPR ceiling.

  python -m dgps_with_iwvi_amd.kernel_resources [--write profiles/<tag>_kernel_resources.txt]
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import yaml

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libiwvi_hip.so")
LLVM_BIN = os.environ.get("IWVI_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size", "max_flat_workgroup_size")

# kernels whose instantiations must not touch scratch memory at all ...
# (k_lik_*: csrc/likelihood_tail.hip -- twenty quadrature nodes unrolled per element: no scratch, and a VGPR ceiling each, MAX_VGPRS below;
#  k_mc_*: csrc/likelihood_multiclass.hip -- twenty running products per sample, which must stay in registers;
#  k_xl_*: csrc/likelihood_explink.hip -- closed forms, and a float64 lgamma / digamma of the shape per wave.
#  k_bo_*: csrc/likelihood_bounded.hip -- Beta and Ordinal, the type a template argument (8 / 9): rolled node loops over erfc / lgamma / digamma.
#  The *_elbo and *_elbo_bwd kernels of the four files are ONE core each, csrc/likelihood_common.h: elbo_points / elbo_bwd_point, inlined over a
#  policy per family -- but for k_lik_elbo_bwd, which keeps a body of its own --: a change to a core moves every family's rows;
#  profiles/likcore_kernel_resources.txt has them side by side)
NO_SCRATCH = ("k_dgp_forward", "k_bw_chain", "k_sample_stats", "k_lik_elbo", "k_lik_elbo_bwd", "k_lik_elem", "k_lik_finish", "k_kde_grid",
              "k_mc_elbo", "k_mc_elbo_bwd", "k_mc_elem", "k_xl_elbo", "k_xl_elbo_bwd", "k_xl_elem",
              "k_lik_mix", "k_mc_mix", "k_xl_mix",
              "k_bo_elbo", "k_bo_elbo_bwd", "k_bo_elem", "k_bo_mix",
              "k_hg_elbo", "k_hg_elbo_bwd", "k_hg_elem", "k_hg_mix",   # csrc/likelihood_hetero.hip: closed forms; the density's twenty nodes unrolled
              "k_lik_sample",          # csrc/likelihood_sample.hip: the type a template argument; rejection loops whose lanes leave at different rounds
              "k_sghmc_step",         # csrc/sghmc.hip: the sampler's update, replayed 10 000 times per evaluation (56 VGPRs today)
              # csrc/cvae.hip: a map's weights travel in registers (32 / 64 per lane) between LDS stagings; they must stay there
              "k_cvae_rows", "k_cvae_wgrad", "k_cvae_finish", "k_cvae_sample",
              # csrc/kmeans.hip: a lane's one or two points travel in registers as float64 (up to 64 doubles per lane at D = 32)
              "k_km_init", "k_km_step", "k_km_update",
              # csrc/bound_family.hip: the MIWAE / CIWAE / VR-alpha reduction and heads -- segmented scans over a chunk's lanes, float64 sums
              "k_bound_logw", "k_bound_bwd", "k_bound_finish",
              # csrc/sample_scores.hip: the sort of k_sample_stats (csrc/sample_sort.h) with other sums; csrc/energy_score.hip: a row sample
              # travels in up to 32 registers through the whole pair loop
              "k_sample_scores", "k_energy_score",
              # csrc/psis.hip: that sort again, then a float64 generalized-Pareto fit whose operands live in LDS, not in per-lane arrays
              "k_psis_summary")
# ... except these (demangled-name substring -> bytes of scratch it is known to use; lower it when a kernel improves)
ALLOWED_SCRATCH = {
    # round 6 (profiles/r06_kernel_resources.txt): every BIG variant (some layer with M > 128: configs[3] / [4]) and every float64-route
    # variant is at ZERO scratch and 178-228 VGPRs since the thread index is made opaque again at every phase boundary (FW_REBASE in
    # csrc/dgp_forward.hip: the lane-dependent tile addresses are formed in the phase that uses them instead of living -- ~80 registers --
    # across the whole layer loop).  Left: a few spilled VGPRs in two narrow M <= 128 variants no BASELINE config takes and in the value +
    # gradient variant of the headline stack (the same rebase there costs the headline 1 %: measured, LABNOTES.md); none may grow.
    # (template arguments: NS, S16, BIG, LEAN_MODE, F64)
    "k_dgp_forward<2,true,false,0,false>": 16, "k_dgp_forward<4,true,false,0,false>": 56,
    "k_dgp_forward<5,true,false,2,false>": 12,
}
# spill counts that may not GROW (demangled-name substring -> (max vgpr spills, max sgpr spills)).  Round 6: the factorisation's column loop
# exists once per role (csrc/precompute_dev.h: chol_blocks), the kernel compiles to 118 VGPRs without a spilled VGPR or a byte of scratch
# (128 VGPRs, 35 spilled, 104 B until then); the SGPR spills (v_writelane into a VGPR, no memory) are what is left of its 1024-thread budget
MAX_SPILLS = {
    "k_precompute": (0, 760),
}


# VGPR ceilings (kernel name before its template arguments -> most VGPRs any instantiation may use).  The likelihood-tail kernels are latency
# chains of transcendental evaluations: 128 VGPRs keep four waves on a SIMD (512 per lane) to hide them.  Today: k_lik_elbo 80, k_lik_elbo_bwd 115,
# k_lik_elem 17-65, k_lik_finish 12, k_mc_elbo 108, k_mc_elbo_bwd 126, k_mc_elem 72-78; the predictive-mixture kernels
# (iwvi_lik_predict_mixture) k_lik_mix 106-110, k_mc_mix 113.
# The exp-link kernels (k_xl_*) do a handful of FMAs and one exp per element: their ceilings are the compiled counts (k_xl_elbo 79-89,
# k_xl_elem 37-63, k_xl_mix 95; k_xl_elbo_bwd 65 when the ceiling was set, 54 today) rounded up to a multiple of 8, so a change that costs them
# a wave of occupancy shows.
# The bounded-target kernels (k_bo_*) likewise: k_bo_elbo 52-68, k_bo_elbo_bwd 68-117, k_bo_elem 34-50, k_bo_mix 68-88 (Ordinal - Beta).
# The heteroskedastic-Gaussian kernels (k_hg_*) likewise, compiled counts rounded up to a multiple of 8: k_hg_elbo 56, k_hg_elbo_bwd 50,
# k_hg_elem 34-63 (the log-space density), k_hg_mix 111-116 (that density inside the point loop with its float64 sums).
# The sampling kernel (k_lik_sample<type>, iwvi_lik_sample_y) is at the family's 128: 16-32 VGPRs for every type but the Poisson, whose
# float64 acceptance test takes 69 (165 with the library's float64 lgamma in it, which is why log k! is a table and a Stirling series there).
# The bound-family kernels (csrc/bound_family.hip), compiled counts rounded up to a multiple of 8: k_bound_logw 74-94, k_bound_bwd 122,
# k_bound_finish 12.
MAX_VGPRS = {"k_lik_elbo": 128, "k_lik_elbo_bwd": 128, "k_lik_elem": 128, "k_lik_finish": 32,
             "k_mc_elbo": 128, "k_mc_elbo_bwd": 128, "k_mc_elem": 128,
             "k_xl_elbo": 96, "k_xl_elbo_bwd": 72, "k_xl_elem": 64,
             "k_lik_mix": 128, "k_mc_mix": 128, "k_xl_mix": 96,
             "k_bo_elbo": 72, "k_bo_elbo_bwd": 120, "k_bo_elem": 56, "k_bo_mix": 88,
             "k_hg_elbo": 56, "k_hg_elbo_bwd": 56, "k_hg_elem": 64, "k_hg_mix": 120,
             "k_lik_sample": 128,
             "k_sghmc_step": 64,
             "k_bound_logw": 96, "k_bound_bwd": 128, "k_bound_finish": 16}


def csrc_hash():
    """sha256 over the kernel sources (csrc/*.hip, csrc/*.h, include/iwvi_hip.h; names and contents, sorted): what a committed PMC
    profile is OF -- comparable on the GPU box, where there is no git history (profiles/traffic_latest.json: `csrc_sha256`)."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(_HERE, "csrc")
    files = sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith((".hip", ".h")))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "iwvi_hip.h"))
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def _readable(name):
    """`_ZN4iwvi13k_dgp_forwardILi5ELb1ELb0ELi1EEEvNS_6FwArgsE` -> `k_dgp_forward<5,true,false,1>` (no c++filt in the image: the kernel
    name and its integral / bool template arguments are all the guard needs)."""
    m = re.match(r"_ZN4iwvi(\d+)", name)
    if not m:
        m2 = re.match(r"_Z(\d+)", name)
        if not m2:
            return name
        n = int(m2.group(1))
        return name[m2.end():m2.end() + n]
    n = int(m.group(1))
    base, rest = name[m.end():m.end() + n], name[m.end() + n:]
    if not rest.startswith("I"):
        return base
    args = []
    for kind, neg, val in re.findall(r"L([ib])(n?)(\d+)E", rest[:rest.index("EE") + 1] if "EE" in rest else rest):
        args.append(("true" if val == "1" else "false") if kind == "b" else ("-" if neg else "") + val)
    return "%s<%s>" % (base, ",".join(args))


def kernel_table(lib_path=LIB_PATH):
    """[{name, demangled, vgpr_count, ...}] for every kernel of every gfx950 code object bundled in ``lib_path``."""
    objdump, readelf = os.path.join(LLVM_BIN, "llvm-objdump"), os.path.join(LLVM_BIN, "llvm-readelf")
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        raise RuntimeError("llvm-objdump / llvm-readelf not found under %s (set IWVI_LLVM_BIN)" % LLVM_BIN)
    tmp = tempfile.mkdtemp(prefix="iwvi_cobj_")
    try:
        so = os.path.join(tmp, "lib.so")                          # (the bundles are extracted next to the input file)
        shutil.copy(lib_path, so)
        subprocess.run([objdump, "--offloading", so], capture_output=True, check=True, cwd=tmp)
        rows = []
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" not in f:
                continue
            notes = subprocess.run([readelf, "--notes", os.path.join(tmp, f)], capture_output=True, text=True, check=True).stdout
            if "---" not in notes:
                continue
            doc = notes[notes.index("---") + 3:]
            doc = doc[:doc.rindex("...")] if "..." in doc else doc
            meta = yaml.safe_load(doc) or {}
            for k in meta.get("amdhsa.kernels", []):
                row = {"symbol": k[".symbol"]}
                for fld in FIELDS:
                    row[fld] = int(k.get("." + fld, 0))
                rows.append(row)
        rows = [r for r in rows if "symbol" in r]
        for r in rows:
            r["name"] = r["symbol"][:-3] if r["symbol"].endswith(".kd") else r["symbol"]
        for r in rows:
            r["demangled"] = _readable(r["name"])
        return rows
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def check(rows=None):
    """Raise AssertionError naming every kernel over its budget; returns the table."""
    rows = kernel_table() if rows is None else rows
    bad = []
    seen = {k: 0 for k in NO_SCRATCH}
    for r in rows:
        d = r["demangled"]
        for k in NO_SCRATCH:
            if d == k or d.startswith(k + "<"):
                seen[k] += 1
                allowed = ALLOWED_SCRATCH.get(d, 0)
                if r.get("private_segment_fixed_size", 0) > allowed:
                    bad.append("%s: %d B of scratch per lane (allowed %d; %d VGPR / %d SGPR spills)" % (
                        d, r["private_segment_fixed_size"], allowed, r.get("vgpr_spill_count", 0), r.get("sgpr_spill_count", 0)))
        cap = MAX_VGPRS.get(d.split("<")[0])
        if cap is not None and r.get("vgpr_count", 0) > cap:
            bad.append("%s: %d VGPRs (budget %d)" % (d, r.get("vgpr_count", 0), cap))
        for s, (mv, ms) in MAX_SPILLS.items():
            if s == d and (r.get("vgpr_spill_count", 0) > mv or r.get("sgpr_spill_count", 0) > ms):
                bad.append("%s: %d VGPR / %d SGPR spills (budget %d / %d)" % (d, r.get("vgpr_spill_count", 0), r.get("sgpr_spill_count", 0), mv, ms))
    for k, n in seen.items():
        if n == 0:
            bad.append("no instantiation of %s found in the library (metadata not read?)" % k)
    assert not bad, "kernel register budget:\n  " + "\n  ".join(bad)
    return rows


def format_table(rows):
    def short(d):
        return d
    out = ["%-64s %5s %5s %5s %6s %6s %8s %8s" % ("kernel", "vgpr", "agpr", "sgpr", "v.spl", "s.spl", "scratchB", "ldsB")]
    for r in sorted(rows, key=lambda r: r["demangled"]):
        out.append("%-64s %5d %5d %5d %6d %6d %8d %8d" % (short(r["demangled"])[:64], r.get("vgpr_count", 0), r.get("agpr_count", 0),
                                                          r.get("sgpr_count", 0), r.get("vgpr_spill_count", 0), r.get("sgpr_spill_count", 0),
                                                          r.get("private_segment_fixed_size", 0), r.get("group_segment_fixed_size", 0)))
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    rows = kernel_table()
    text = format_table(rows)
    if len(sys.argv) > 2 and sys.argv[1] == "--write":
        open(sys.argv[2], "w").write(text)
    sys.stdout.write(text)
    check(rows)
