"""One row per ``k_dgp_forward`` instantiation (csrc/dgp_forward.hip: ``fw_variants[]``): the tail, the variant word the call must produce
(``iwvi_debug_last_forward_variant``: ns | S16 << 8 | BIG << 9 | LEAN << 10 | SHP << 11 | F64 << 12) and the smallest call that selects it.
Plain data: nothing here touches a device.  tests/test_forward_variant_cases_host.py proves the table complete against
tests/golden/fw_plan.npz and plans every row; tests/test_gpu_forward_variants.py runs the runnable rows against the float64 oracle.

Every stack is ``synthetic.make_spec(L=2, Dx=8, Dy=1, R=...)``: an inner SharedMixedMok layer (D = 8, R latent GPs mixed to P = 8, Linear mean
function) feeding a plain final layer (D = 8, R = P = 1).  D = 8 > 3 keeps ``settings.f64_stage1 = "auto"`` off every layer that is not
flagged on purpose; it is make_spec's default and the width at which the suite states its per-sample log-weight tolerance, which follows
the conditioning of K_uu: MAX_DIAG_RATIO bounds max / min of diag(Lm) of every stack by the largest value recorded for the 8-D BASELINE
stacks (``DGP_VI.autotune_f64``).  make_spec puts the inducing points of both layers on X[:M], so every row takes its data from the END of
the spec's 2341 rows (``data_rows``): a point that is itself an inducing point would feed zeros to every block of the solve but its own.
What selects each dimension of the table:

  ns     by T alone (ns = ceil(T / 4096), capped at 5, made odd for the predictive tails; no development option).
         bound tail: K = 7, B = 11, 586, 1171, 1756, 2341 -> T = 77, 4102, 8197, 12292, 16387 -> ns = 1..5.  7 divides none of 16, 32, 48,
         64, 80, so data points straddle workgroups; the last chunk holds 13, 6, 37, 4, 67 samples.
         predictive / sampling tails: N = 13, S = 7, 631, 1261 -> N S = 91, 8203, 16393 -> ns = 1, 3, 5; the last chunk holds 11, 43, 73
         samples and S divides no chunk.
  S16    on: an even number of 16-row blocks in every GP layer (M = 32, 160, 256); off: an odd number (M = 48, 144, 272).
  BIG    M > 128: M = 144 / 160 (9 / 10 blocks, one column at a time) and, as a second case of the same word, M = 272 / 256 (17 / 16 blocks:
         the super-block solve, whose blocking SBD / SBT changes with NS).  R = 2 there keeps the float64 oracle of 16 393 rows quick.
  F64    ``GPLayer.f64_stage1 = True`` on the first GP layer (the F64 variants are built with BIG and fp32 stage 2).
  LEAN / SHP (0x405, 0x505, 0x805, 0x905): the headline shapes compiled in.  tests/test_gpu_lean_variant.py compares them per sample with
         the oracle; they are listed with the covering test and ``run=False``."""
import collections

TAIL_BOUND, TAIL_PREDICT, TAIL_SAMPLE = 0, 1, 2              # _abi.FW_TAIL_*
TAIL_NAMES = {TAIL_BOUND: "bound", TAIL_PREDICT: "predict", TAIL_SAMPLE: "sample"}
S16, BIG, LEAN, SHP, F64 = 1 << 8, 1 << 9, 1 << 10, 1 << 11, 1 << 12

DX, DY, L = 8, 1, 2
MAX_DIAG_RATIO = 85.0                                       # max / min of diag(Lm) of every GP layer of every stack (see above)
# name -> make_spec's M and R, the flag of the first GP layer, the bits of the word
STACKS = collections.OrderedDict([
    ("m32", dict(M=32, R=3, f64=False, bits=S16)),
    ("m48", dict(M=48, R=3, f64=False, bits=0)),
    ("m160", dict(M=160, R=3, f64=False, bits=S16 | BIG)),
    ("m256", dict(M=256, R=2, f64=False, bits=S16 | BIG)),
    ("m144", dict(M=144, R=3, f64=False, bits=BIG)),
    ("m272", dict(M=272, R=2, f64=False, bits=BIG)),
    ("m32f64", dict(M=32, R=3, f64=True, bits=F64 | BIG)),
])
BOUND_K = 7
BOUND_B = {1: 11, 2: 586, 3: 1171, 4: 1756, 5: 2341}        # ns -> B
PREDICT_N = 13
PREDICT_S = {1: 7, 3: 631, 5: 1261}                          # ns -> S
SPEC_B = max(BOUND_B.values())                               # one spec (and one device model) per stack serves every row of it

# tail, word, stack (None: not run here), ns, (B, K) of the bound tail or (N, S) of the others, run, covering test of a row not run
Row = collections.namedtuple("Row", "tail word stack ns shape run covered_by")


def spec_kwargs(stack):
    """``synthetic.make_spec``'s arguments for a stack of the table."""
    s = STACKS[stack]
    return dict(L=L, M=s["M"], B=SPEC_B, K=BOUND_K, Dx=DX, Dy=DY, R=s["R"], seed=700 + s["M"] + (1 if s["f64"] else 0), n_data=SPEC_B)


def rows():
    out = []
    for name, s in STACKS.items():
        for ns, B in BOUND_B.items():
            out.append(Row(TAIL_BOUND, ns | s["bits"], name, ns, (B, BOUND_K), True, None))
        for tail in (TAIL_PREDICT, TAIL_SAMPLE):
            for ns, S in PREDICT_S.items():
                out.append(Row(tail, ns | s["bits"], name, ns, (PREDICT_N, S), True, None))
    # (that test evaluates through LEAN, then reads the same noise step back with per-layer outputs, which takes SHP -- both words and
    # identical log-weights asserted -- and holds them to the oracle per sample; its "fp32 stage 2" case covers the two words without S16)
    cover = "tests/test_gpu_lean_variant.py::test_shapes_inside_the_variant_take_it_and_match_the_oracle"
    out += [Row(TAIL_BOUND, 5 | mode | s16, None, 5, None, False, cover) for mode in (LEAN, SHP) for s16 in (0, S16)]
    return out


ROWS = rows()
RUNNABLE = [r for r in ROWS if r.run]


def data_rows(n):
    """The rows of the spec's X and Y that a call on n points reads: the last n (beyond every inducing point while n <= SPEC_B - max M)."""
    return slice(SPEC_B - n, SPEC_B)


def row_id(r):
    return "%s-%#x-%s" % (TAIL_NAMES[r.tail], r.word, r.stack)


def total_rows(r):
    """T of the launch."""
    return r.shape[0] * r.shape[1]
