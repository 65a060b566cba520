"""Cases, fp64 references, statistics and DERIVED bars of the aggregator forward's fp32-feature routes (csrc/agg_f3.h, agg_f2.h,
agg_hs.h, agg_split.h behind ops.agg_forward), shared by tests/test_agg_precision_host.py (the bars are reachable by plain
fp32 arithmetic, see every one-plane variant from at least 8 bars away, and the inputs are tie-free) and
tests/test_agg_precision_gpu.py (the kernels meet them on every route).  Nothing here is tuned on a GPU or taken from the code
under test; the reference is oracle/agg_oracle.py's milnet_forward in fp64.

u = 2^-24: half a unit in the last place of fp32, relative to the value.  All roundings are to nearest even.

HOW ERRORS ARE COMBINED.  A worst-case bound that is linear in the number of roundings (trunk32_cases' 3 K u S) is useless here:
through K = 512, 128 hidden units and 128 query units it is ~1e-3 on a score, ABOVE the error of a kernel that lost a whole
plane (1.4e-4 .. 1.8e-3), because a one-plane operand's 2^-12 relative errors add up like a random walk too.  So the errors of
the chain are split into two kinds and carried to the score by the chain's own first-order coefficients (from the fp64 reference):
  det   a fixed function of the data that may be one-sided — what an operand's planes do not hold, a dropped plane product, the
        truncation of a bf16 cut, fast_tanh's hardware exp / rcp: worst case, |coefficient| x bound, added up.  Where both
        factors of such a term are known here (the features' and the weights' planes) the term is FORMED, with its signs, and
        only what is not known (the planes of the kernel's own hidden layer) is bounded;
  rand  the roundings of fp32 additions, fmas and products: each at most u x |the value rounded|, independent and of either
        sign.  n of them with bounds b_i enter as LAM sqrt(sum (coefficient_i b_i)^2), LAM = 4: by Hoeffding's inequality a sum
        of independent errors inside +-b_i exceeds that with probability < 2 exp(-LAM^2 / 2) = 7e-4 at the worst, and a rounding
        error spread evenly over +-b has standard deviation b / sqrt(3), which makes the bar 6.9 standard deviations (1e-11 per
        value).  |The value rounded| is a partial sum: it is bounded from the kernel's order of additions, not by the whole
        sum of absolute values.
1.01 pays for the second-order terms.

OPERANDS, two-plane fp16 routes "f16x2" (k_attend_f3, k_attend_f2).  x' = x 2^e per ROW (max |x'| in [2^13, 2^14): f2_scale from
the row maximum k_logits_stream left), h0 = rne16(x'), h1 = rne16(x' - h0); the weights likewise with ONE scale per tensor
(k_pack_agg_f2).  What the planes do not hold, r = x' - h0 - h1 (at most 2 u |x'| while h1 is normal, 2^-25 absolutely below
that), and the dropped product h1 w1 (at most 4 u |x w|) are formed HERE from the same cuts in numpy (np.float16 rounds to
nearest even and keeps subnormals), so small rows and small weights carry their true floor and not a quoted one:
    det_H[n, j] = | sum_k r_x w + x r_w + h1_x h1_w |          (in unscaled units; r_x r_w is second order)
The kept products have at most 22 significant bits: exact in fp32.
OPERANDS, three-plane bf16 routes "bf16x3" (k_attend_hs, k_query_attend_split; NP = 6).  v = h + m + l by truncation is exact;
of the nine products (m, l), (l, m), (l, l) are dropped, each below 2^-20 (1 + 2^-8) |x w| in sum.  From the same cuts:
    det_H[n, j] = | sum_k m_x l_w + l_x m_w + l_x l_w |

ACCUMULATION OVER K (GEMM 1).  Each of the NPROD = 3 (f16x2) or 6 (bf16x3) plane products is an MFMA of its own over WIN = 32
(v_mfma_f32_16x16x32_f16, k_attend_f3; k_attend_f2's is 16) or 16 k (v_mfma_f32_32x32x16_bf16) into the same fp32 accumulator;
how an MFMA orders and rounds its WIN additions is not documented: at most one rounding per product added, in any order inside
the window, the windows in k order (agg_f3.h "the steps in k order"; the split kernels walk 16-k steps).  With P the fp64
prefix of x . w at the window borders and S_s = sum over window s of |x| |w|: the MFMA of the main product (h0 w0; h h) rounds
partial sums below |P_(s-1)| + S_s; an MFMA of a small product (at most 2^-7 of the main one) moves the accumulator by less
than S_s / 64 and rounds values below max(|P_(s-1)|, |P_s|) + S_s / 64 wherever it stands among the window's MFMAs:
    rand_H[n, j]^2 = u^2 (WIN sum_s ((|P_(s-1)| + S_s)^2 + (NPROD - 1) (max(|P_(s-1)|, |P_s|) + S_s / 64)^2) + pre^2)
(pre^2: the un-scaling fma with the bias).  ReLU keeps or zeroes: the coefficient of a hidden unit is 0 where the reference's
pre-activation is below -(det_H + LAM rand_H).

HIDDEN LAYER (GEMM 2): rand_z as rand_H with H for x, W2 for W1.  H is cut from the kernel's OWN fp32 value, so its planes are
bounded, W2's are formed; an error e_j of hidden unit j's operand reaches the score through all 128 query units at once, with
cF[j] = sum_j2 g[j2] W2[j2, j] (g below) — the sum over j2 is taken with its signs before the absolute value:
    f16x2:  |rho_j| <= 2 u H_j + floor (what two rounded planes miss; k_attend_f3 scales by a BOUND of the row's maximum,
            max_j ||W1[j]||_1 max|x| + max|b1|: 2^-25 of a scale that maps this bound below 2^14, < 2^-37 of the bound),
            |h1_j| <= 2^-11 (1 + 2^-10) H_j times the known low plane w1 of W2, H_j times the known residue r_w of W2:
            det_2 = sum_j H_j (2 u |cF[j]| + 2^-11 (1 + 2^-10) |sum_j2 g[j2] w1[j2, j]| + |sum_j2 g[j2] r_w[j2, j]|) + floor sum_j |cF[j]|
    bf16x3: 0 <= m_j < 2^-7 H_j, 0 <= l_j < 2^-14 H_j (truncation of H >= 0) times the known planes of W2:
            det_2 = sum_j H_j (2^-7 |sum_j2 g[j2] l_w[j2, j]| + 2^-14 |sum_j2 g[j2] (m_w + l_w)[j2, j]|)

fast_tanh(z) = 1 - 2 rcp(1 + exp2(z c)), c = 2 log2(e) in fp32 (agg_common.h).  t = z c: c's rounding and the product's, 2 u |t|,
which is 2 u ln2 |t| = 4 |z| u relative on e = exp2(t); v_exp_f32 and v_rcp_f32 are 1 ulp (2 u) each, 1 + e one rounding.  With
r = 2 / (1 + e) = 1 - q:  |dr| <= r ((4 |z| + 2) u e / (1 + e) + 3 u), and r e / (1 + e) = (1 - q^2) / 2, then the rounding of 1 - r:
    b_tanh = u ((2 |z| + 1) (1 - q^2) + 3 (1 - q) + 1)            (5 u absolute at z = 0, 7 u at q = -1, u at q = +1)
det (a fixed function of z), carried to the score as sum_j b_tanh[j] |q_max[j]| / sqrt(128).

SCORE s = Q . q_max / sqrt(128).  A lane adds the units it holds by sequential fmas, then a fixed tree (_chains: attend_tail
two chains of 64 and one exchange; attend_tail_hs and f2_tail eight chains of 16 and three levels; k_attend_f3 sixteen chains
of 8 and four levels).  A chain's fma rounds a partial sum below the chain's prefix of |Q_j q_max[j]| / sqrt(128), the squared
bounds of one tree level add up to at most S^2 = (sum_j |Q_j q_max[j]| / sqrt(128))^2; then the product with 1 / sqrt(128):
    rand_s^2 = u^2 (sum over chains and positions of prefix^2 + levels S^2 + s^2)      (the larger of the kind's two kernels)

CRITICAL QUERY q_max (qmax_block, plain fp32): lane (k / 4) mod 64 adds its x_m[k] W1[j, k] by sequential fmas (partial sums
below the lane's own sum of absolute values), six levels of a 64-lane sum (at most S1^2 per level, S1 = sum_k |x_m| |W1| +
|b1|), the bias; layer 2: a product and an fma per lane, the lane sum, the bias, below S2; tanhf 2 ulp (4 u |q|).  Its error is
shared by all rows of the bag and enters the log-attention of row i through (Q_i - Q_m) / sqrt(128) (rand_q).

LOG-ATTENTION, row i against the critical row m, class c:  log(A_i / A_m) = s_i - s_m (the normalisation cancels).  With
g_i[j2] = q_max[j2] (1 - Q_i[j2]^2) / sqrt(128) (through tanh) and c_i[j] = cF_i[j] where the ReLU passes:
    det_i    = sum_j |c_i[j]| det_H[i, j] + det_2 + sum_j2 b_tanh[i, j2] |q_max[j2]| / sqrt(128)
    rand_i^2 = sum_j c_i[j]^2 rand_H[i, j]^2 + sum_j2 g_i[j2]^2 rand_z[i, j2]^2 + rand_s^2
    L_i = 1.01 (det_i + det_m + LAM sqrt(rand_i^2 + rand_m^2 + rand_q,i^2)) + 2 (R + 3) u
Last term: A = expf(s - m) / l (k_finish): the argument's rounding, u |s - m| with |s - m| <= R = 2 sum_j |q_max[j]| / sqrt(128)
whatever reference m a kernel subtracts (a tile's maximum; the bag's constant bound in k_attend_f3), expf 1 ulp, the product
with 1 / l one rounding — for row i and for row m.  The statistic is max_i |error_i| / L_i per bag and class.

sum_i A_i.  l is summed from the attend kernels' own expf values (rescaled by expf of the tile references: again (R + 3) u),
A is formed from a second expf of the stored score: 2 (R + 3) u, and the additions of l and the rescaled merges of k_finish
(fixed order: sequential runs, 64-lane sums, four waves — no path longer than 40 additions for the bags here, N <= 2^14):
    bar_sumA = 1.01 (2 (R + 3) + 40) u.

B[c, k] = sum_i A_i v_ik.  To first order dB_k = sum_i A_i (v_ik - B_k) ds_i (softmax): row i's own score error with the
coefficient A_i (v_ik - B_k) — det and the shared q_max part linearly, rand in quadrature over the rows.  The value rows are read
as fp32 (bf16x3: exact) or from the row-scaled planes (f16x2: 2 u, floor 2^-37 of the row maximum), the weight p / (row scale)
is one fp32 value (u), the normalisation is bar_sumA; then N_ACC(N) fmas and additions on the longest path (f16x2: two per row,
a wave's quarter of the rows in sequence, N / 2 + 24 with the merges; bf16x3: 32 rows in sequence, waves, k_finish's walk: 64).
With T[c, k] = sum_i A_i |v_ik| (the scale the B error is relative to):
    bar_B[c, k] = 1.01 (sum_i A_i |v_ik - B_k| (det_i + LAM rand_q,i) + LAM sqrt(sum_i A_i^2 (v_ik - B_k)^2 rand_i^2)
                        + (bar_sumA + (c_v + 1 + LAM sqrt(N_ACC)) u) T[c, k] + floor)
pred[o] = fcc_b[o] + sum_ck fcc_w[o, c, k] B[c, k] (k_finish: products, 64-lane sums; k_pred: Kv / 64 x C partials in sequence):
    bar_pred[o] = sum_ck |fcc_w[o, c, k]| bar_B[c, k] + 1.01 LAM sqrt(8 + C Kv / 64) u (sum_ck |fcc_w| T + |fcc_b[o]|)
classes (k_logits_stream: lane (k / 4) mod 8 adds its terms by sequential fmas, three exchanges, the bias; k_logits_argmax,
K % 4 != 0: 64 lanes, six levels), with S = sum_k |x_k| |w_k| + |b|, as for q_max:
    bar_classes = 1.01 LAM u sqrt(sum over lanes of (chain length) (lane's sum of |x w|)^2 + (levels + 1) S^2)
The critical index is exact: the cases are tie-free — the reference's top two logits of a class differ by at least 100 bars
(a seeded bag that comes closer than 200 is drawn again, make_case_bag).

WHICH BAR WHERE.  "f16x2" for attend = f3 and f2, "bf16x3" for attend = hs and split (route_kind).  They differ in det_H and
det_2 (what two rounded fp16 planes miss and drop against three dropped products of exact planes), in NPROD and WIN (3 MFMAs of
32 k against 6 of 16 per MAC), in the score's chains and in the value rows (planes / fp32).  On the cases here the bf16x3 bar on
the log-attention is 5 to 8 % above the f16x2 bar (median over the rows of a case).  The host test holds every degraded variant to 8 bars of BOTH."""
import functools

import numpy as np

import agg_oracle as orc
from inputs import make_bag
from util import load_weights

U = 2.0 ** -24
LAM = 4.0
ISQ = 1.0 / np.sqrt(128.0)
KINDS = ("f16x2", "bf16x3")
NPROD = {"f16x2": 3, "bf16x3": 6}
WIN = {"f16x2": 32, "bf16x3": 16}          # k of one MFMA: v_mfma_f32_16x16x32_f16 (k_attend_f3; k_attend_f2 16) / v_mfma_f32_32x32x16_bf16
STATS = ("logatt", "sumA", "B", "pred", "classes")

SETS = [(128, 1), (512, 1), (512, 2), (384, 2), (256, 5), (166, 1), (1024, 2), "tcga"]
# the bags of the 32-row regime: (rows, flavour); "s1" / "s3": make_bag at scale 1 / 3, "spread": rows times 10^U(-1, 1)
SMALL = [(1, "s1"), (31, "s3"), (33, "spread"), (64, "s1"), (65, "s3"), (400, "s1"), (400, "spread")]
# the batch of the 128-row regime: 54 runs of the short lengths, a 400-row bag behind every 14th run from the 7th on
SHORT = [1, 15, 16, 17, 31, 32, 33, 47]
FLAVOURS = ("s1", "s3", "spread")


# Bag seeds are moved per weight set where the first choice left a (case, variant) pair below 8 bars (host test, check 2):
# with the tcga weights a one-plane W2 sits 6 .. 8 bars away on most seeded bags, 10 on these.
SEED_SHIFT = {"tcga": 400}


def batch_layout():
    out = []
    for r in range(54):
        out += [(n, FLAVOURS[(r + i) % 3]) for i, n in enumerate(SHORT)]
        if r % 14 == 6:
            out.append((400, FLAVOURS[(r // 14) % 3]))
    return out


BATCH = batch_layout()          # 436 bags, 11 968 rows: 11968 / 128 + 436 = 529.5 >= 512
LAYOUTS = {"small": SMALL, "batch": BATCH}


def route_kind(attend):
    return {"f3": "f16x2", "f2": "f16x2", "hs": "bf16x3", "split": "bf16x3"}[attend]


def set_name(s):
    return s if isinstance(s, str) else f"K{s[0]}_C{s[1]}"


@functools.lru_cache(maxsize=None)
def weights(s):
    """Weight set `s`: the shipped "tcga" set, or the seeded (K, C) set in the style of test_f3_shape_gpu._weights."""
    if isinstance(s, str):
        return {k: np.asarray(v, np.float32) for k, v in load_weights(s).items()}
    K, C = s
    rng = np.random.default_rng(4100 + K + C)
    w = {"fc_w": rng.normal(0, 0.05, (C, K)), "fc_b": rng.normal(0, 0.05, (C,)), "q0_w": rng.normal(0, 0.06, (128, K)),
         "q0_b": rng.normal(0, 0.05, (128,)), "q2_w": rng.normal(0, 0.08, (128, 128)), "q2_b": rng.normal(0, 0.05, (128,)),
         "fcc_w": rng.normal(0, 0.05, (C, C, K)), "fcc_b": rng.normal(0, 0.05, (C,))}
    return {k: v.astype(np.float32) for k, v in w.items()}


def dims(s):
    w = weights(s)
    return w["q0_w"].shape[1], w["fc_w"].shape[0]


def classes_bar(x, w):
    """(fp64 instance logits, bar_classes) [n, C] (the docstring's last paragraph)."""
    x = np.asarray(x, np.float64)
    fw, fb = np.asarray(w["fc_w"], np.float64), np.asarray(w["fc_b"], np.float64)
    K = x.shape[1]
    S = np.abs(x) @ np.abs(fw).T + np.abs(fb)
    lanes = 8 if K % 4 == 0 else 64                              # k_logits_stream / k_logits_argmax
    return x @ fw.T + fb, 1.01 * LAM * U * np.sqrt(_lanes_rand2(x[:, None, :] * fw[None, :, :], lanes, 0) + S ** 2)


def tie_margin(x, w):
    """The smallest gap between the reference's top two logits of a class, in units of 100 bars (>= 1: tie-free)."""
    classes, bar = classes_bar(x, w)
    if len(classes) == 1:
        return np.inf
    top = np.sort(classes, axis=0)
    return float(np.min((top[-1] - top[-2]) / (100 * bar.max(axis=0))))


@functools.lru_cache(maxsize=None)
def make_case_bag(s, layout_name, i):
    """Bag i of layout "small" / "batch" for weight set s, fp32 [n, K].  A seeded bag whose top two logits of a class come
    closer than 200 bars is drawn again from the next seed (the host test asks for 100)."""
    K, _ = dims(s)
    n, flavour = LAYOUTS[layout_name][i]
    seed = 4100 + 7 * K + 1000 * (layout_name == "batch") + i + SEED_SHIFT.get(s, 0)
    while True:
        x = make_bag(seed, n, K, 3.0 if flavour == "s3" else 1.0)
        if flavour == "spread":
            f = 10.0 ** np.random.default_rng(seed + 50000).uniform(-1.0, 1.0, (n, 1))
            x = (x * f.astype(np.float32)).astype(np.float32)
        if tie_margin(x, weights(s)) >= 2.0:
            x.setflags(write=False)
            return x
        seed += 100000


# ---- the chain in fp64 with hooks (the degraded variants), and in plain fp32 ------------------------------------------------
def r16(a):
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def rb16(a):
    """round to nearest even to bf16 (finite inputs)"""
    v = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    v = ((v + 0x7FFF + ((v >> 16) & 1)) >> 16) << 16
    return v.astype(np.uint32).view(np.float32).astype(np.float64)


VARIANTS = {   # name: (the place that is rounded once, the rounding, the statistic it touches)
    "x_f16": ("x", r16, "logatt"), "W1_f16": ("W1", r16, "logatt"), "H_f16": ("H", r16, "logatt"), "W2_f16": ("W2", r16, "logatt"),
    "H_bf16": ("H", rb16, "logatt"), "vals_f16": ("vals", r16, "B"), "xlogits_f16": ("xlogits", r16, "classes"),
}


def chain64(x, w, variant=None):
    """(classes, pred, A, B, idx) as agg_oracle.milnet_forward(dtype="f64") computes them, one operand rounded once."""
    place, rnd, _ = VARIANTS[variant] if variant else (None, None, None)
    f = lambda name, a: rnd(a) if place == name else a          # noqa: E731
    x = np.asarray(x, np.float64)
    p = {k: np.asarray(v, np.float64) for k, v in w.items()}
    classes = f("xlogits", x) @ p["fc_w"].T + p["fc_b"]
    idx = np.argmax(classes, axis=0)

    def q(rows):
        h = f("H", np.maximum(f("x", rows) @ f("W1", p["q0_w"]).T + p["q0_b"], 0))
        return np.tanh(h @ f("W2", p["q2_w"]).T + p["q2_b"])
    s = (q(x) @ q(x[idx]).T) * ISQ
    e = np.exp(s - s.max(axis=0, keepdims=True))
    A = e / e.sum(axis=0, keepdims=True)
    B = A.T @ f("vals", x)
    pred = np.einsum("ock,ck->o", p["fcc_w"], B) + p["fcc_b"]
    return classes, pred[None], A, B[None], idx


def fast_tanh32(z):
    """agg_common.h's fast_tanh in fp32: 1 - 2 / (1 + exp2(z * 2 log2(e)))"""
    z = np.asarray(z, np.float32)
    with np.errstate(over="ignore"):
        e = np.exp2(z * np.float32(2.8853900817779268))
    return np.float32(1) - np.float32(2) * (np.float32(1) / (np.float32(1) + e))


def chain32(x, w):
    """The same chain in plain fp32 numpy (every operand and intermediate fp32, fast_tanh restated)."""
    x = np.asarray(x, np.float32)
    p = {k: np.asarray(v, np.float32) for k, v in w.items()}
    classes = x @ p["fc_w"].T + p["fc_b"]
    idx = np.argmax(classes, axis=0)

    def q(rows):
        h = np.maximum(rows @ p["q0_w"].T + p["q0_b"], np.float32(0))
        return fast_tanh32(h @ p["q2_w"].T + p["q2_b"])
    s = (q(x) @ q(x[idx]).T) * np.float32(ISQ)
    e = np.exp(s - s.max(axis=0, keepdims=True))
    A = e / e.sum(axis=0, keepdims=True, dtype=np.float32)
    B = A.T @ x
    pred = np.einsum("ock,ck->o", p["fcc_w"], B) + p["fcc_b"]
    assert classes.dtype == A.dtype == B.dtype == pred.dtype == np.float32
    return classes, pred[None], A, B[None], idx


# ---- the cuts, as the kernels make them ----------------------------------------------------------------------------------------
def f2_scale(m):
    """The power of two s with m s in [2^13, 2^14) (agg_f2.h f2_scale; 1 for m == 0)."""
    m = np.asarray(m, np.float64)
    e = np.floor(np.log2(np.where(m > 0, m, 1.0)))
    return np.where(m > 0, 2.0 ** np.clip(13 - e, -125, 125), 1.0)


def cut_f16x2(a, scale):
    """What the planes miss and the low plane (both signed) of a (fp32 values) cut at `scale`, in unscaled units."""
    s = np.asarray(a, np.float64) * scale
    with np.errstate(over="raise"):
        h0 = s.astype(np.float16).astype(np.float64)
        h1 = (s - h0).astype(np.float16).astype(np.float64)
    return (s - h0 - h1) / scale, h1 / scale


def cut_bf16x3(a):
    """m and l (signed) of the truncating three-plane cut of fp32 values (agg_split.h split3)."""
    a = np.ascontiguousarray(a, np.float32)
    h = (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    r1 = a - h
    m = (r1.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    return m.astype(np.float64), (r1 - m).astype(np.float64)


def _windows(a, b, win):
    """a [n, k], b [j, k] -> over the win-k windows s (win = the k of one MFMA): sum (|P_(s-1)| + S_s)^2 and sum (max(|P_(s-1)|, |P_s|) + S_s / 64)^2,
    [n, j] each (the partial sums of the main plane product's MFMA and of a small one's: see the docstring)."""
    n, k = a.shape
    nb = -(-k // win)
    ap = np.zeros((n, nb * win))
    ap[:, :k] = a
    bp = np.zeros((b.shape[0], nb * win))
    bp[:, :k] = b
    a3 = ap.reshape(n, nb, win).transpose(1, 0, 2)
    b3 = bp.reshape(-1, nb, win).transpose(1, 2, 0)
    blk = a3 @ b3                                   # [nb, n, j]
    cum = np.cumsum(blk, axis=0)
    prev = np.abs(cum - blk)
    S = np.abs(a3) @ np.abs(b3)
    return ((prev + S) ** 2).sum(axis=0), ((np.maximum(prev, np.abs(cum)) + S / 64) ** 2).sum(axis=0)


def _lanes_rand2(t, nlanes, extra):
    """Rounding variance bound (in u^2) of a sum of the terms |t| [.., k] formed as the fp32 kernels form it: lane (k // 4) %
    nlanes adds its terms by sequential fmas (every partial sum below the lane's own sum of |t|), then log2(nlanes) levels of
    pairwise additions (the squared partial bounds of one level sum to at most S^2) and `extra` more roundings of the whole."""
    k = t.shape[-1]
    per = 4 * nlanes
    rounds = -(-k // per)
    tp = np.zeros(t.shape[:-1] + (rounds * per,))
    tp[..., :k] = np.abs(t)
    lane = tp.reshape(t.shape[:-1] + (rounds, nlanes, 4)).sum(axis=(-3, -1))     # [.., nlanes]
    S = lane.sum(axis=-1)
    return 4 * rounds * (lane ** 2).sum(axis=-1) + (np.log2(nlanes) + extra) * S ** 2


def qmax_rand2(xm, Hm, W1, b1, W2, b2):
    """The critical query's own rounding variances (the docstring's CRITICAL QUERY; qmax_block, and the backward's qrow_body,
    which adds in the same order): of the hidden pre-activations and of the query pre-activations z, [C, 128] each, for the
    critical rows xm [C, K] and their hidden layer Hm [C, 128] (fp64)."""
    S1m = np.abs(xm) @ np.abs(W1).T + np.abs(b1)
    S2m = np.abs(Hm) @ np.abs(W2).T + np.abs(b2)
    rq_H2 = U * U * (_lanes_rand2(xm[:, None, :] * W1[None, :, :], 64, 0) + S1m ** 2)
    rq_z2 = U * U * (_lanes_rand2(Hm[:, None, :] * W2[None, :, :], 64, 0) / 2 + (6 + 1) * S2m ** 2)
    return rq_H2, rq_z2


def _chains(kernel):
    """The query units a lane adds up by sequential fmas, in its order, and the tree levels behind (agg_common.h attend_tail,
    agg_hs.h attend_tail_hs = agg_f2.h f2_tail, agg_f3.h): [groups, chain] unit indices, levels."""
    if kernel == "tail":      # lane half hi: units 32 t + 8 g + 4 hi + e in (t, g, e) order; one exchange
        return np.array([[32 * t + 8 * g + 4 * hi + e for t in range(4) for g in range(4) for e in range(4)] for hi in range(2)]), 1
    if kernel == "hs":        # wave w, half hi: units 32 w + 8 q + 4 hi + e; one exchange, then ((a + b) + (c + d))
        return np.array([[32 * w + 8 * q + 4 * hi + e for q in range(4) for e in range(4)] for w in range(4) for hi in range(2)]), 3
    # f3: wave w, lane group g: units ubase + 8 uh + e, ubase = 32 w + 16 (g >> 1) + 4 (g & 1); sixteen partials in a four-level tree
    return np.array([[32 * w + 16 * (g >> 1) + 4 * (g & 1) + 8 * uh + e for uh in range(2) for e in range(4)]
                     for w in range(4) for g in range(4)]), 4


DOT_KERNELS = {"f16x2": ("hs", "f3"), "bf16x3": ("tail", "hs")}


def _dot_rand2(t, kind):
    """Rounding variance bound (in u^2) of the score's dot product over the terms t [n, 128] = Q_j q_max[j] / sqrt(128): every
    fma of a lane's chain rounds a partial sum below the chain's prefix of |t|, every tree level adds at most S^2 = (sum |t|)^2;
    the larger of the two kernels of the kind."""
    at = np.abs(t)
    S2 = at.sum(axis=1) ** 2
    best = 0.0
    for kernel in DOT_KERNELS[kind]:
        units, levels = _chains(kernel)
        pre = np.cumsum(at[:, units], axis=2)                   # [n, groups, chain]
        best = np.maximum(best, (pre ** 2).sum(axis=(1, 2)) + levels * S2)
    return best


# ---- reference and bars of one bag ---------------------------------------------------------------------------------------------
class Ref:
    """The fp64 reference of one bag, and per route kind the bars: L [n, C], sumA [C], B [C, K], pred [C], classes [n, C]."""


_WCUTS = {}


def _weight_cuts(w):
    """The plane cuts of W1 and W2 of weight dict w (signed, fp64), made once per weight set."""
    key = id(w["q0_w"])
    if key not in _WCUTS:
        a1, a2 = f2_scale(np.abs(w["q0_w"]).max()), f2_scale(np.abs(w["q2_w"]).max())
        _WCUTS[key] = (w["q0_w"], cut_f16x2(w["q0_w"], a1), cut_f16x2(w["q2_w"], a2), cut_bf16x3(w["q0_w"]), cut_bf16x3(w["q2_w"]))
    return _WCUTS[key][1:]


def reference(x, w, kinds=KINDS):
    x32 = np.asarray(x, np.float32)
    x = x32.astype(np.float64)
    p = {k: np.asarray(v, np.float64) for k, v in w.items()}
    W1, b1, W2, b2 = p["q0_w"], p["q0_b"], p["q2_w"], p["q2_b"]
    n, K = x.shape
    C = p["fc_w"].shape[0]
    r = Ref()
    r.n, r.K, r.C = n, K, C
    r.out = orc.milnet_forward(x32, w, dtype="f64")            # THE reference: (classes, pred, A, B, idx)
    classes, pred, A, B, idx = r.out
    pre = x @ W1.T + b1
    H = np.maximum(pre, 0)
    z = H @ W2.T + b2
    Q = np.tanh(z)
    qm = Q[idx]                                                 # [C, 128]
    s = (Q @ qm.T) * ISQ
    assert np.allclose(np.exp(s - s.max(0)) / np.exp(s - s.max(0)).sum(0), A, rtol=1e-12, atol=0)
    ax = np.abs(x)
    _, r.bar_classes = classes_bar(x32, w)
    r.tie_margin = tie_margin(x32, w)
    # what both kinds share
    rowmax = ax.max(axis=1, keepdims=True)
    b_tanh = U * ((2 * np.abs(z) + 1) * (1 - Q * Q) + 3 * (1 - Q) + 1)
    Rc = 2 * np.abs(qm).sum(axis=1) * ISQ                                      # [C]
    r.bar_sumA = 1.01 * (2 * (Rc + 3) + 40) * U
    # the critical query's own error (plain fp32): per class, per hidden / query unit
    xm = x[idx]                                                 # [C, K]
    Hm = H[idx]
    rq_H2, rq_z2 = qmax_rand2(xm, Hm, W1, b1, W2, b2)                                          # [C, 128] each
    T = A.T @ ax                                                # [C, K]
    r.kind = {}
    (rw, w1), (rw2, w12), (wmid, wlo), (wmid2, wlo2) = _weight_cuts(w)
    for kind in kinds:
        if kind == "f16x2":
            rx, x1 = cut_f16x2(x32, f2_scale(rowmax))
            det_H = np.abs(rx @ W1.T + x @ rw.T + x1 @ w1.T)
            hfloor = 2.0 ** -37 * (np.abs(W1).sum(axis=1).max() * rowmax + np.abs(b1).max())        # [n, 1]
        else:
            xmid, xlo = cut_bf16x3(x32)
            det_H = np.abs(xmid @ wlo.T + xlo @ wmid.T + xlo @ wlo.T)
        nsm, win = NPROD[kind] - 1, WIN[kind]
        win1, win1s = _windows(x, W1, win)
        win2, win2s = _windows(H, W2, win)
        rand_H2 = U * U * (win * (win1 + nsm * win1s) + pre ** 2)
        mask = pre > -(det_H + LAM * np.sqrt(rand_H2))
        rand_z2 = U * U * (win * (win2 + nsm * win2s) + z ** 2)
        k = Ref()
        k.L, k.det, k.rand2, k.randq2 = (np.zeros((n, C)) for _ in range(4))
        for c in range(C):
            g = qm[c]
            G = g[None, :] * (1 - Q * Q) * ISQ                  # [n, 128]
            cF = G @ W2
            cH = cF * mask
            if kind == "f16x2":
                det2 = (H * (2 * U * np.abs(cF) + 2.0 ** -11 * (1 + 2.0 ** -10) * np.abs(G @ w12) + np.abs(G @ rw2))).sum(1) \
                    + (np.abs(cF) * hfloor).sum(1)
            else:
                det2 = (H * (2.0 ** -7 * np.abs(G @ wlo2) + 2.0 ** -14 * np.abs(G @ (wmid2 + wlo2)))).sum(1)
            k.det[:, c] = (np.abs(cH) * det_H).sum(1) + det2 + (b_tanh @ np.abs(g)) * ISQ
            k.rand2[:, c] = (cH ** 2 * rand_H2).sum(1) + (G ** 2 * rand_z2).sum(1) \
                + U * U * (_dot_rand2(Q * g[None, :] * ISQ, kind) + s[:, c] ** 2)
            # the critical query's error, through (Q_i - Q_m) / sqrt(128)
            m = int(idx[c])
            E = (Q - Q[m][None, :]) * ISQ
            Em = E * (1 - g * g)[None, :]
            cq = (Em @ W2) * (pre[m] > 0)[None, :]
            k.randq2[:, c] = (cq ** 2 * rq_H2[c][None, :]).sum(1) + (Em ** 2 * rq_z2[c][None, :]).sum(1) \
                + ((E * (4 * U * np.abs(g))[None, :]) ** 2).sum(1)
            k.L[:, c] = 1.01 * (k.det[:, c] + k.det[m, c] + LAM * np.sqrt(k.rand2[:, c] + k.rand2[m, c] + k.randq2[:, c])) \
                + 2 * (Rc[c] + 3) * U
        n_acc = n / 2 + 24 if kind == "f16x2" else 64
        c_v = 2.0 if kind == "f16x2" else 0.0
        floor_B = 2.0 ** -37 * (A * rowmax).sum(axis=0) if kind == "f16x2" else np.zeros(C)
        k.bar_B = np.zeros((C, K))
        for c in range(C):
            dev = np.abs(x - B[0, c][None, :])                  # [n, K]: dB_k = sum_i A_i (v_ik - B_k) ds_i to first order
            a = A[:, c]
            k.bar_B[c] = 1.01 * ((a * (k.det[:, c] + LAM * np.sqrt(k.randq2[:, c]))) @ dev
                                 + LAM * np.sqrt((a * a * k.rand2[:, c]) @ (dev * dev))
                                 + (r.bar_sumA[c] + (c_v + 1 + LAM * np.sqrt(n_acc)) * U) * T[c] + floor_B[c])
        aw = np.abs(p["fcc_w"])
        k.bar_pred = np.einsum("ock,ck->o", aw, k.bar_B) + 1.01 * LAM * np.sqrt(8 + C * K / 64) * U * (
            np.einsum("ock,ck->o", aw, T) + np.abs(p["fcc_b"]))
        r.kind[kind] = k
    return r


def ratios(got, r, kind):
    """Worst error / bar of every statistic for outputs got = (classes [n, C], pred [1, C] or [C], A [n, C], B [.., C, K], idx [C])
    of the bag with reference r; "idx": whether the critical index is the reference's."""
    classes, pred, A, B, idx = [np.asarray(t) for t in got]
    rc, rp, rA, rB, ridx = r.out
    k = r.kind[kind]
    out = {"idx": bool(np.array_equal(np.asarray(idx).reshape(-1), ridx))}
    out["classes"] = float((np.abs(classes.astype(np.float64) - rc) / r.bar_classes).max())
    A = A.astype(np.float64)
    out["sumA"] = float((np.abs(A.sum(axis=0) - 1.0) / r.bar_sumA).max())
    cols = np.arange(r.C)
    with np.errstate(divide="ignore", invalid="ignore"):
        la = np.log(A / A[ridx, cols][None, :]) - np.log(rA / rA[ridx, cols][None, :])
    la[ridx, cols] = 0.0
    out["logatt"] = float((np.abs(la) / k.L).max()) if np.all(np.isfinite(la)) else float("inf")
    out["B"] = float((np.abs(B.astype(np.float64).reshape(r.C, -1) - rB.reshape(r.C, -1)) / k.bar_B).max())
    out["pred"] = float((np.abs(pred.astype(np.float64).reshape(-1) - rp.reshape(-1)) / k.bar_pred).max())
    return out


@functools.lru_cache(maxsize=None)
def small_case(s):
    """[(x, Ref)] for the bags of SMALL with weight set s."""
    return [(x, reference(x, weights(s))) for x in (make_case_bag(s, "small", i) for i in range(len(SMALL)))]
