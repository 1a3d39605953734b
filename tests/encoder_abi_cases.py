"""The cases of tests/test_encoder_abi_gpu.py and the dispatcher's predicates mirrored per case, in a module of their own: the GPU test
runs them, and tests/test_encoder_plan_cpu.py holds the mirror against what csrc/encoder_plan.h decides -- without a GPU."""
import pytest

from tests import encoder_abi_ref as R

KNOBS = ("GENNBV_CONV_SPLIT", "GENNBV_SPLITX", "GENNBV_SPLITX_MAXWG", "GENNBV_WGRAD_DMA", "GENNBV_CONV_MAXWG", "GENNBV_FUSED_BWD",
         "GENNBV_CONV1_SPLIT", "GENNBV_FUSED_TRAIN", "GENNBV_FUSED_EVAL", "GENNBV_ANALYTIC_BN1")


def K(g, b, inp="rows", ac=None, env=None, train=True, feats=True, fill="rand", dfeat="randn", force=False, skip=False, prep=0,
      big=False):
    """inp: "rows" fp32 observation rows at the policy's row stride, "i8" the same plus aligned int8 rows, "compact" int8 rows only
    (obs_grid NULL), "unaligned" fp32 rows whose grid slice is 4 bytes off 16-byte alignment.  ac: None, "rows" (per-row
    autocorrelation) or "total" (+ autocorr_total)."""
    env = dict(env or {})
    parts = [f"g{g}", f"b{b}", inp] + ([f"ac-{ac}"] if ac else []) + [f"{k[7:].lower()}={v}" for k, v in env.items()]
    parts += [s for s, on in (("eval", not train), ("nofeat", not feats), (f"fill-{fill}", fill != "rand"), (f"df-{dfeat}", dfeat != "randn"),
                              ("force_fp32", force), ("skip", skip), (f"prep{prep}", prep), ("big", big)) if on]
    return pytest.param(dict(g=g, b=b, inp=inp, ac=ac, env=env, train=train, feats=feats, fill=fill, dfeat=dfeat, force=force,
                             skip=skip, prep=prep, big=big), id="-".join(parts))


NOFT = {"GENNBV_FUSED_TRAIN": "0"}
CASES = [
    # ---- shape classes on their default paths ----
    K(7, 3),                     # O2 = 1; odd row stride: the generic conv1 / conv1-weight-gradient kernels
    K(7, 1, "compact"),          # B = 1 at P2 = 1: a BN-2 count of 1
    K(8, 2),                     # O2 = 1; LDS-staged fp32 conv1
    K(16, 9, "i8", ac="rows"),   # analytic BN1 + fused fp32 backward; 9 samples: dead slots of the XCD item mapping
    K(20, 3),
    K(20, 9),
    K(32, 2),                    # LDS-staged fp32 conv1 weight gradient, one row request and two input requests per lane
    K(33, 2),                    # even O1 (16): the odd-parity slot 15 holds data
    K(48, 2, "i8", ac="total"),
    K(63, 2),                    # split conv2 kernels, generic conv1 (G % 4 != 0), fp32 data gradient
    K(64, 3, "i8", ac="rows"),   # the default training path: one-launch conv1 + conv2
    K(64, 9, "i8"),              # measured BN1; the fused backward computes the autocorrelation total itself
    K(64, 2),                    # LDS-staged fp32 conv1 and conv1 weight gradient beside the split conv2 kernels
    K(64, 2, "unaligned"),       # generic conv1 and conv1-weight-gradient kernels beside the split conv2 kernels
    K(64, 2, "compact", ac="rows"),
    K(64, 128, "i8", ac="total"),  # the benchmark's minibatch
    K(65, 2),                    # split, even O1 = 32 (slot 15 of the odd half row is data)
    K(66, 1, "compact"),
    K(68, 2),                    # x-tiled: one 16-output tile whose 17th even voxel is data
    K(80, 2, "i8", ac="rows"),   # x-tiled, partial last tile; fused x-tiled data gradient with NA = 20
    K(100, 2),                   # x-tiled, partial last tiles; split weight gradient beside the fp32 data gradient
    K(128, 3, "i8", ac="rows"),
    K(128, 1),
    K(130, 1),                   # x-tiled, even O1 = 64
    K(131, 1),                   # the first fp32 fallback above the split range
    # ---- knobs (read by the library on every call) ----
    K(64, 2, "i8", ac="rows", env={"GENNBV_CONV_SPLIT": "0"}),
    K(128, 1, "i8", ac="rows", env={"GENNBV_CONV_SPLIT": "0"}),
    K(64, 2, "i8", ac="rows", env={"GENNBV_SPLITX": "1", **NOFT}),
    K(64, 2, "i8", ac="rows", env={"GENNBV_SPLITX": "1", "GENNBV_SPLITX_MAXWG": "8", **NOFT}),
    K(128, 2, "i8", ac="rows", env={"GENNBV_SPLITX_MAXWG": "8"}),
    K(64, 3, "i8", ac="rows", env={"GENNBV_WGRAD_DMA": "0"}),
    K(64, 3, "i8", ac="rows", env={"GENNBV_CONV_MAXWG": "512"}),
    K(64, 2, "i8", ac="rows", env={"GENNBV_FUSED_BWD": "0"}),
    K(128, 1, "i8", ac="rows", env={"GENNBV_FUSED_BWD": "0"}),
    K(16, 2, "i8", env={"GENNBV_FUSED_BWD": "0"}),   # int8-staged conv1 weight gradient, one row request per lane
    K(80, 1, "i8", env={"GENNBV_FUSED_BWD": "0"}),   # the same with four
    K(64, 2, "i8", ac="rows", env={"GENNBV_CONV1_SPLIT": "0"}),
    K(64, 2, "i8", ac="rows", env=NOFT),
    K(64, 2, "i8", ac="rows", force=True),
    K(128, 1, "i8", ac="rows", force=True),
    # ---- modes ----
    K(20, 3, train=False),
    K(64, 3, "i8", train=False),
    K(64, 3, "i8", train=False, prep=1),
    K(64, 3, "i8", train=False, env={"GENNBV_FUSED_EVAL": "0"}),
    K(128, 2, "i8", train=False),
    K(64, 2, "i8", ac="rows", feats=False),
    K(128, 1, "i8", ac="rows", feats=False),
    K(20, 2, skip=True),
    K(64, 2, "i8", ac="rows", skip=True),
    # ---- edges ----
    K(20, 2, fill="zeros"),
    K(64, 2, "i8", ac="rows", fill="zeros"),
    K(64, 2, "i8", ac="rows", fill="zeros", force=True),
    K(64, 2, "i8", fill="ones"),
    K(128, 1, "i8", ac="rows", fill="ones"),
    K(20, 2, dfeat="zero"),
    K(64, 2, "i8", ac="rows", dfeat="zero"),
    K(128, 1, "i8", ac="rows", dfeat="zero"),
    K(20, 3, dfeat="onehot"),
    K(64, 2, "i8", ac="rows", dfeat="onehot"),
    K(64, 2, "i8", ac="rows", big=True),
    K(128, 1, "i8", ac="rows", big=True),
]


# ------------------------------------------------------------------------------------------------------------------------------
# the dispatcher's predicates (csrc/encoder.hip), mirrored to state per case what is written and which arithmetic runs
def _paths(cs):
    g, env = cs["g"], cs["env"]
    off = lambda k: env.get(k, "")[:1] == "0"  # noqa: E731
    o1 = R.out_size(g)
    o2, xh = R.out_size(o1), (o1 + 1) // 2
    i8 = cs["inp"] in ("i8", "compact")
    sx = env.get("GENNBV_SPLITX", "")
    split = not off("GENNBV_CONV_SPLIT") and not cs["force"] and xh == 16 and o2 <= 15
    splitx = (not off("GENNBV_CONV_SPLIT") and not cs["force"] and o2 >= 1 and sx[:1] != "0"
              and ((16 < xh <= 32 and o2 <= 32) or (xh == 16 and o2 <= 15 and sx[:1] == "1")))
    fused_bwd = not off("GENNBV_FUSED_BWD") and i8 and g % 16 == 0 and 3 * g * g <= 65536
    i8_staged = i8 and g % 16 == 0 and 3 * (2 * o1 + 1) * g * 4 <= 65536 and 2 * o1 + 1 <= g
    analytic = cs["train"] and cs["ac"] is not None and i8_staged and 3 * g * g <= 65536 and not off("GENNBV_ANALYTIC_BN1")
    fused_eval = not cs["train"] and split and i8_staged and g == 64 and not off("GENNBV_FUSED_EVAL")
    fused_train = analytic and split and g == 64 and not off("GENNBV_CONV1_SPLIT") and not off("GENNBV_FUSED_TRAIN")
    return dict(split_fwd=split or splitx or fused_eval or fused_train, split_wg=split or splitx, split_dg=fused_bwd and (split or splitx),
                fused_bwd=fused_bwd, analytic=analytic, fused_eval=fused_eval)
