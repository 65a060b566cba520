"""Cases, per-stage fp64 references and DERIVED bars of the fp32 aggregator backward (csrc/agg_bwd.hip, agg_bwd_bags.h, agg_gx.h
behind ops.agg_backward / ops.agg_backward_bags), shared by tests/test_agg_bwd_precision_host.py (the bars are reachable by a
numpy restatement of every stage and by plain fp32, and every mutant of the restatement misses the bar of the stage it touches) and
tests/test_agg_bwd_precision_gpu.py (the kernels meet them).  Nothing here is tuned on a GPU or taken from the code under test.

WHY STAGE BY STAGE.  The backward leaves every intermediate in its workspace, each in a region that nothing overwrites
(bwd_layout; dsmil_agg_backward_layout answers the offsets): gB, D, q_max, g_q, gA, gs, gz2, H, Q, gH, the per-tile partials of g_q
and the row-range partials of the weight gradients.  So every launch is compared with fp64 applied to ITS OWN inputs as the device
holds them: both operands of every contraction are known bit for bit (a cut's dropped products are FORMED, with their signs), the
ReLU mask is the device's own H (no entry is left out), and no error is carried from one stage to the next — no cancellation in
gA - D, no mask flips, no cuts of values only the kernel knows.  A stage's outputs are the next stage's inputs and the last stages'
outputs are the gradients, so tight stage bars plus the loose end-to-end tests (tests/test_agg_bwd_gpu.py and its siblings) cover
the sequence.  ("dev" below: read from the workspace or from the call's outputs.)

u = 2^-24, LAM = 4 and the 1.01 second-order factor are tests/agg_precision_cases.py's (its docstring: HOW ERRORS ARE COMBINED), and
so are the two kinds of error:
  det   what a three-plane cut drops.  v = h + m + l by truncation is exact (agg_split.h split3), the kernels keep six of the nine
        plane products, smallest first ((l,h), (h,l), (m,m), (m,h), (h,m), (h,h): S3_PA / S3_PB from q = 3 on) and drop (m,l),
        (l,m), (l,l).  Both operands are known here, always:   det = | sum_k m_a l_b + l_a m_b + l_a l_b |.
  rand  fp32 roundings, each at most u times the partial sum it rounds, in quadrature times LAM.  The partial sums follow the
        kernel's own order of additions.
A plane contraction (stages 4a, 6, 7, 10: v_mfma_f32_32x32x16_bf16, six MFMAs per 16-k window into one fp32 accumulator, the
windows in k order) takes agg_precision_cases._windows with WIN = 16, NPROD = 6, as the forward's GEMM 1 does:
    rand^2 = u^2 (16 sum_s ((|P_(s-1)| + S_s)^2 + 5 (max(|P_(s-1)|, |P_s|) + S_s / 64)^2) [+ (value after the bias)^2])
    bar    = 1.01 (det + LAM rand)
A sequential fp32 sum or fma chain ("chain") rounds its own prefix: rand^2 = u^2 sum_i P_i^2 (a separately rounded product adds
t_i^2); a fixed pairwise tree adds the squares of its partial sums level by level.  Chains of a handful of classes are added
linearly (u sum_c |P_c|) instead: they are too short for a statistical bound.

THE STAGES (the kernel's order was read from the source named; one bag / batch of bags).
 1  k_bwd_prep block 0 / k_bags_prep, k_bwd_prep blocks 1.. / k_bags_head.
    gB[c,k] = g_B + sum_o g_pred[o] fcc_w[o,c,k]: an fma chain over o from g_B.                    rand, chain over o
    D[c]: thread t of 256 adds gB_dev[c,k] B[c,k] for k = t, t + 256, .. and then A[n,c] g_A[n,c] for n = t, t + 256, .. by fmas;
    block_sum_256: four DPP levels in a 16-lane row, two over the rows, two over the waves.         rand, chains + 8 S^2 (S = sum_t |thread's sum|)
    g_fcc_w = g_pred[o] B[c,k]: one rounding (bar 1.01 u |ref|); g_fcc_b = g_pred: bit-equal.  Batch: both are sums over the bags
    in bag order (k_bags_head), a chain over b with separately rounded products.
 2  k_fc / k_bags_ga: gA = V gB_dev^T.  agg_precision_cases.classes_bar with W := gB_dev, b := 0 (the FCLayer kernel).
 3  k_bwd_qrow / k_bags_qrow (qrow_body): q_max = q(x[idx]) in plain fp32, the forward's qmax_block order.  The forward's
    critical-query rule (agg_precision_cases.qmax_rand2) gives the variances of the hidden and the query pre-activations; carried
    to q through W2 where the ReLU passes (|relu a - relu b| <= |a - b|) and through tanh: bar = 1.01 (LAM (1 - q^2) rand_z + 4 u |q|)
    (tanhf: 2 ulp); the linear query is the hidden layer itself: 1.01 LAM rand_H.
 4a k_bwd_rows_hs / k_bwd_rows (mlp_tile_hs, mlp_tile_split, mlp_tile_split_dma: the same planes, products and k order).
    H = relu(x W1^T + b1): plane contraction over K of x and W1, both cut here; + pre^2 for the bias.  Compared with relu of the
    fp64 pre-activation: ReLU is 1-Lipschitz, so the bar of the pre-activation holds for H on every entry.
    Q = fast_tanh(H_dev W2^T + b2): plane contraction over 128 of H_dev's OWN cut and W2's; then through tanh and fast_tanh's own
    bound (agg_precision_cases: b_tanh):   bar_Q = 1.01 ((1 - q^2) bar_z + b_tanh).  Linear query: Q is the pre-activation.
 4b the tile kernels' tail.  gs = A ((gA_dev + g_A) - D_dev) * fl(1/sqrt(128)): four roundings, linearly:
        bar_gs = 1.01 u (|A| / sqrt(128) (|ga| + |ga - D|) + 2 |gs|).
    gqp[tile, c, j] = sum over the 32 rows of a tile of gs_dev[n,c] Q_dev[n,j]: a rounded product per row, then five levels of
    halving over the half-wave (halfwave_colsum64 / 16: lanes l and l ^ 16, then ^ 8, 4, 2, 1).    rand, products + the tree's partials
 5  k_bwd_critical / k_bags_critical (critical_body).  g_q[c,j]: group g of eight adds the tiles g, g + 8, .. in order
    (sum_parts16), then ((0+1)+(2+3))+((4+5)+(6+7)).                                                rand, chains + tree
    gz2 (the tile kernels' store, completed here): G = fma chain over the classes of gs_dev[n,c] q_max_dev[c,j]; t = fl(1 - fl(q q))
    (two roundings: u q^2 + u t; an fma would be one); gz2 = fl(G t); at row idx_c, classes in order, gz2 += g_q_dev[c] t.  Linearly:
        bar = 1.01 u (t sum_c |P_c| + |G| (q^2 + t) + |G t|  +  sum over the row's classes (|g_q| (q^2 + t) + |g_q t| + |value so far|)).
    The linear query has t = 1 and no product.
 6  k_bwd_gh_hs / k_bwd_gh: gH = (gz2_dev W2) [H_dev > 0]: plane contraction over 128 of gz2_dev's cut and W2's (the zero bias
    adds nothing); where H_dev <= 0 the entry is exactly 0.
 7  k_tn_split, per ROW RANGE s (rows s R .. of the N rows; R, S from the layout query): part0[s] = A0[range]^T x[range]
    (A0 = gH_dev; gz2_dev for the linear query), part1[s] = gz2_dev[range]^T H_dev[range]: plane contractions over the range's rows,
    16-row windows in row order.  A whole-N contraction hides a lost product behind its own random walk (see the numbers below); a
    range of a few hundred rows does not.  pb0 / pb1[s] = column sums of A0 / gz2: a thread adds the rows of its 8-row group(s) of
    every 32-row step in row order, then a pairwise tree — four chains (group (n mod 32) / 8) and two levels on 16-B aligned rows
    with K % 4 == 0 (WIDE), else two chains (groups {0, 2} and {1, 3}) and one level.                    rand, chains + tree
 8  k_bwd_reduce: g_W1, g_b1, g_W2, g_b2 = the sums of the ranges' partials in range order (sum_parts16).      rand, chain over s
    k_tn_small + k_reduce_parts (dense g_classes): part[s, c, k]: wave w of four adds g_classes[n,c] x[n,k] over n = first + w,
    + 4, .. (rounded product, rounded sum), then (0+1)+(2+3); part_b the same over g_classes; g_fc_w / g_fc_b = their sums in range
    order, then the sparse term g_max[c] x[idx_c] (+ g_max[c]) added — bag by bag in a batch.            rand for the sums, the sparse terms linearly
 9  k_bwd_gvals / k_bags_gvals: g_vals[n,k] = sum_c A[n,c] gB_dev[c,k], a C-term chain: bar = 1.01 u sum_c (|P_c| + |t_c|).
10  k_bwd_gx / k_bags_gx (agg_gx.h): g_x = L_dev W1 (L = gH_dev; gz2_dev for the linear query): plane contraction over 128, then
    per class v = fma(g_classes[n,c] (+ g_max[c] at row idx_c: one rounding), Wf[c,k], v), v = fma(A[n,c], gB_dev[c,k], v) (v =
    Identity only): the tail's partial sums join the contraction's rand in quadrature.

The statistic is max over the checked elements of |got - ref| / bar per stage; a stage passes at <= 1.  A non-finite value, a
non-zero masked entry or an error against a zero bar counts as infinity.

CASES.  Weight sets and bags are agg_precision_cases' (weights, make_case_bag; SMALL = 1, 31, 33, 64, 65, 400, 400 rows in three
flavours); the 17-row bag of the batch and the 65 600-row bag are drawn here (make_rows).  The upstream gradients are dense on
pred, classes, A and B plus a sparse g_max, seeded per case.  The critical index is an INPUT of the backward (the forward's output),
so no case depends on a tie.

CPU NUMBERS (tests/test_agg_bwd_precision_host.py on the cases up to 400 rows; error / bar, worst case and stage):
  a  the six-product restatement of every stage on the 36 cases up to 400 rows (the batch included), worst case per stage:
     1: gB 0.37, D 0.03, g_fcc_w 0.99 (one rounding against 1.01 u), g_fcc_b 0.17;  2: 0.28;  3: 0.24;  4a: H 0.10, Q 0.49;
     4b: gs 0.84, gqp 0.44;  5: g_q 0.34, gz2 0.96 (the linear bounds are attained to a few per cent);  6: 0.12;
     7: partials 0.18, column sums 0.46;  8: sums over the ranges 0.56, k_tn_small's partials 0.47, g_fc_w 0.91;  9: 0.56;  10: 0.43.
     A plain float32 matmul in the plane stages: 4a H 0.17, 6 0.17, 7 0.16, 10 0.43.
  b  mutants, smallest .. largest over the cases, on the stage they touch:
     one operand on its high plane      4a 583 .. 2603,  6 883 .. 2867,  7 2336 .. 3929,  10 1773 .. 2373
     one product dropped, (h,l) (l,h) (m,m)   4a 2.3 .. 11.3,  6 3.0 .. 11.6,  7 8.8 .. 25.9,  10 6.5 .. 11.4   (no seed was moved)
     (1 - Q^2) from bf16 Q 2.1e4 .. 6.4e4;  g_q left out at the critical rows 9.0e5 .. 1.7e7;  D without sum A g_A 3.4e3 .. 3.4e5.
     Stage 10 has no mutant at ONE row: A = 1 there, gA + g_A - D cancels to its own roundings, gH is rounding noise and the
     contraction's share of g_x lies under the roundings of the class tail (the host test asserts that this is the reason).
  c  65 600 rows, (K, C) = (128, 1), R = 704, S = 94: range 40 restated 0.11 of the bar, x on its high plane 1525, a dropped product
     4.8 .. 6.3 bars; the same product dropped from ALL rows taken as one contraction: 2.0 .. 3.1 of that contraction's bar."""
import functools
from typing import NamedTuple

import numpy as np

import agg_precision_cases as ac
from agg_precision_cases import LAM, U, _lanes_rand2, _windows, classes_bar, cut_bf16x3, fast_tanh32, qmax_rand2  # noqa: F401
from inputs import make_bag

QD = 128
SCALE32 = float(np.float32(0.08838834764831845))        # the kernels' 1 / sqrt(128)
F32, F64 = np.float32, np.float64
KEPT = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))   # (plane of a, plane of b) of the six products, smallest first
PLANE_NAME = "hml"
STAGES = ("1", "2", "3", "4a", "4b", "5", "6", "7", "8", "9", "10")


class Case(NamedTuple):
    name: str
    s: object                   # weight set of agg_precision_cases.weights
    bags: tuple                 # ((rows, flavour, index in agg_precision_cases.SMALL or None), ..)
    entry: str                  # "one": ops.agg_backward; "bags": ops.agg_backward_bags
    tile: str                   # the row tile the case is meant to reach (_native.BWD_TILE)
    nonlinear: bool = True
    own_vals: bool = False      # the caller's own value rows and want_g_vals (stages 9, and 2 on vals)
    gx: bool = False            # want_g_feats (stage 10)
    misalign: bool = False      # feats a contiguous view with data_ptr() % 16 == 4
    row_map: bool = False
    sample: bool = False        # the 65 600-row case: stages 4 - 6 on sampled rows, stage 7 on sampled ranges


def _small(i):
    return (ac.SMALL[i][0], ac.SMALL[i][1], i)


HS_SETS = [(512, 2), (128, 1), (1024, 2), (256, 5)]
BATCH_BAGS = tuple(_small(i) for i in range(6)) + ((17, "s3", None),)          # 1, 31, 33, 64, 65, 400, 17 rows
CASES = [Case(f"hs_{ac.set_name(s)}_{ac.SMALL[i][0]}{ac.SMALL[i][1]}", s, (_small(i),), "one", "hs", gx=(s == (512, 2)))
         for s in HS_SETS for i in range(len(ac.SMALL))]
CASES += [
    Case("w1reg_K166_33", (166, 1), (_small(2),), "one", "w1_reg"),
    Case("w1reg_K166_400", (166, 1), (_small(5),), "one", "w1_reg"),
    Case("w1reg_unaligned_K512_65", (512, 2), (_small(4),), "one", "w1_reg", misalign=True),
    Case("w4dma_K128_65600", (128, 1), ((65600, "s1", None),), "one", "w4_dma", sample=True),
    Case("linq_65", "linq", (_small(4),), "one", "hs", nonlinear=False),
    Case("own_vals_K256_C5_65", (256, 5), (_small(4),), "one", "hs", own_vals=True),
    Case("bags_K512_C2", (512, 2), BATCH_BAGS, "bags", "hs", gx=True),
    Case("bags_K166_C1", (166, 1), BATCH_BAGS, "bags", "w1_reg"),
    Case("rowmap_K512_65", (512, 2), (_small(4),), "one", "hs", row_map=True),
]
BY_NAME = {c.name: c for c in CASES}
HOST_CASES = [c for c in CASES if sum(b[0] for b in c.bags) <= 400 or c.entry == "bags"]   # the batch: no bag above 400 rows


def make_rows(s, n, flavour, salt):
    """A bag of n rows for weight set s in agg_precision_cases' flavours (its make_case_bag without the tie rule: the backward takes
    the critical index as an input)."""
    K, _ = ac.dims(s)
    seed = 9100 + 7 * K + salt
    x = make_bag(seed, n, K, 3.0 if flavour == "s3" else 1.0)
    if flavour == "spread":
        f = 10.0 ** np.random.default_rng(seed + 50000).uniform(-1.0, 1.0, (n, 1))
        x = (x * f.astype(F32)).astype(F32)
    return np.ascontiguousarray(x, F32)


@functools.lru_cache(maxsize=None)
def case_rows(name):
    """(x [N, K] fp32 in logical row order, lengths) of a case."""
    c = BY_NAME[name]
    bags = [ac.make_case_bag(c.s, "small", i) if i is not None else make_rows(c.s, n, fl, n) for n, fl, i in c.bags]
    x = np.ascontiguousarray(np.concatenate(bags), F32)
    x.setflags(write=False)
    return x, tuple(len(b) for b in bags)


def case_weights(c):
    w = dict(ac.weights(c.s))
    if not c.nonlinear:
        assert "q2_w" not in w
    return w


@functools.lru_cache(maxsize=None)
def case_vals(name):
    """The caller's own value rows [N, Kv = K] (own_vals): seeded, not the features."""
    c = BY_NAME[name]
    x, _ = case_rows(name)
    v = np.random.default_rng(77 + len(x)).standard_normal(x.shape).astype(F32)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def case_upstream(name):
    """Dense upstream gradients on pred, classes, A, B and the sparse g_max of a case: fp32, seeded."""
    c = BY_NAME[name]
    x, lengths = case_rows(name)
    K, C = ac.dims(c.s)
    nb, N = len(lengths), len(x)
    rng = np.random.default_rng(6200 + N + 13 * C + K)
    g = {"g_pred": 0.5 * rng.standard_normal((nb, C)), "g_max": 0.5 * rng.standard_normal((nb, C)),
         "g_classes": 0.1 * rng.standard_normal((N, C)), "g_A": rng.standard_normal((N, C)),
         "g_B": 0.05 * rng.standard_normal((nb, C, K))}
    g = {k: np.ascontiguousarray(v, F32) for k, v in g.items()}
    for v in g.values():
        v.setflags(write=False)
    return g


class Inp:
    """The inputs of one backward call as the entry sees them (logical row order), and the layout numbers of the call."""


def build_inputs(c, A, B, idx, layout):
    """c: Case; A [N, C], B [nb, C, Kv], idx [nb, C] (bag-local): the forward's outputs, fp32 / int64; layout: the answer of
    _native.backward_layout for the call."""
    x, lengths = case_rows(c.name)
    i = Inp()
    i.case, i.x, i.lengths = c, x, lengths
    i.off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    i.nb, i.N = len(lengths), len(x)
    i.K, i.C = ac.dims(c.s)
    i.w = case_weights(c)
    i.nonlinear = c.nonlinear
    i.identity_v = not c.own_vals
    i.vals = x if i.identity_v else case_vals(c.name)
    i.A, i.B, i.idx = np.asarray(A, F32), np.asarray(B, F32).reshape(i.nb, i.C, -1), np.asarray(idx, np.int64).reshape(i.nb, i.C)
    i.__dict__.update(case_upstream(c.name))
    i.R, i.S, i.splits, i.small_rows = int(layout.R), int(layout.S), int(layout.splits), int(layout.small_rows)
    i.wide = (i.K % 4 == 0) and not c.misalign
    i.one = c.entry == "one"
    i.bag_of = np.repeat(np.arange(i.nb), lengths)
    i.crit = i.off[:-1, None] + i.idx                       # [nb, C] batch rows of the critical instances
    return i


def forward32(x, w, nonlinear):
    """(A, B, idx) of one bag in plain fp32 numpy (v = Identity): what stands in for the forward's outputs on the CPU."""
    x = np.asarray(x, F32)
    p = {k: np.asarray(v, F32) for k, v in w.items()}
    idx = np.argmax(x @ p["fc_w"].T + p["fc_b"], axis=0)

    def q(rows):
        h = rows @ p["q0_w"].T + p["q0_b"]
        return fast_tanh32(np.maximum(h, F32(0)) @ p["q2_w"].T + p["q2_b"]) if nonlinear else h
    s = (q(x) @ q(x[idx]).T) * F32(SCALE32)
    e = np.exp(s - s.max(axis=0, keepdims=True))
    A = (e / e.sum(axis=0, keepdims=True, dtype=F32)).astype(F32)
    return A, (A.T @ x).astype(F32), idx


# ---- arithmetic helpers ----------------------------------------------------------------------------------------------------------
def planes(a):
    """(h, m, l) of the truncating three-plane cut of fp32 values, fp64 each (h + m + l == a exactly)."""
    a = np.ascontiguousarray(a, F32)
    m, lo = cut_bf16x3(a)
    return a.astype(F64) - m - lo, m, lo


def plane_ref(a, b, after=None):
    """a [n, k], b [j, k] fp32 -> (a b^T in fp64, det, rand^2 in absolute units) of the six-product contraction (docstring);
    `after` [j] or None: a bias added behind the contraction (one more rounding, of the sum)."""
    _, am, al = planes(a)
    _, bm, bl = planes(b)
    a64, b64 = np.asarray(a, F64), np.asarray(b, F64)
    ref = a64 @ b64.T
    det = np.abs(am @ bl.T + al @ bm.T + al @ bl.T)
    w1, w1s = _windows(a64, b64, 16)
    rand2 = U * U * 16 * (w1 + 5 * w1s)
    if after is not None:
        ref = ref + np.asarray(after, F64)
        rand2 = rand2 + U * U * ref ** 2
    return ref, det, rand2


def plane_bar(det, rand2):
    return 1.01 * (det + LAM * np.sqrt(rand2))


def mm6(a, b, drop=None, hi_a=False, hi_b=False, plain=False):
    """a b^T as the kernels form it, restated: the six kept plane products of every 16-k window added one by one, smallest
    first, into an fp32 accumulator (one rounding per product and window).  drop: a (plane of a, plane of b) pair left out;
    hi_a / hi_b: that operand reduced to its high plane; plain: a plain float32 matmul instead."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if plain:
        return a @ b.T
    pa, pb = list(planes(a)), list(planes(b))
    if hi_a:
        pa[1], pa[2] = np.zeros_like(pa[1]), np.zeros_like(pa[2])
    if hi_b:
        pb[1], pb[2] = np.zeros_like(pb[1]), np.zeros_like(pb[2])
    acc = np.zeros((a.shape[0], b.shape[0]), F32)
    for k0 in range(0, a.shape[1], 16):
        sl = slice(k0, k0 + 16)
        for i, j in KEPT:
            if (i, j) == drop:
                continue
            acc = (acc.astype(F64) + pa[i][:, sl] @ pb[j][:, sl].T).astype(F32)
    return acc


def tree_rand2(sums):
    """sums [g, ..] (g a power of two) added pairwise, neighbours first: the sum of the squares of every partial sum formed."""
    r2 = 0.0
    while len(sums) > 1:
        sums = sums[0::2] + sums[1::2]
        r2 = r2 + (sums ** 2).sum(axis=0)
    return r2


def halving_rand2(v):
    """v [32, ..] summed by recursive halving (lanes l and l ^ 16, then ^ 8, 4, 2, 1): the squares of every partial sum formed."""
    r2 = 0.0
    while len(v) > 1:
        v = v[:len(v) // 2] + v[len(v) // 2:]
        r2 = r2 + (v ** 2).sum(axis=0)
    return r2


def chains_rand2(v, grp, ng, products=False):
    """v [n, ..] added as ng sequential chains (element i belongs to chain grp[i], in index order) and a pairwise tree over the
    chains: (the sum in fp64, sum of the squared partial sums — every prefix of every chain, the tree's levels, and with
    `products` the terms themselves, which were rounded as products)."""
    v = np.asarray(v, F64)
    r2 = np.zeros(v.shape[1:])
    sums = np.zeros((ng,) + v.shape[1:])
    for g in range(ng):
        vg = v[grp == g]
        if len(vg):
            pre = np.cumsum(vg, axis=0)
            r2 = r2 + (pre ** 2).sum(axis=0)
            sums[g] = pre[-1]
    if products:
        r2 = r2 + (v ** 2).sum(axis=0)
    return sums.sum(axis=0), r2 + tree_rand2(sums)


def chains32(v, grp, ng):
    """The same sum in fp32: sequential chains (np.cumsum adds in order), then the pairwise tree."""
    v = np.asarray(v, F32)
    sums = np.zeros((ng,) + v.shape[1:], F32)
    for g in range(ng):
        vg = v[grp == g]
        if len(vg):
            sums[g] = np.cumsum(vg, axis=0, dtype=F32)[-1]
    while len(sums) > 1:
        sums = sums[0::2] + sums[1::2]
    return sums[0]


def ratio(got, ref, bar, exact0=None):
    """max |got - ref| / bar; inf for a non-finite value, an error against a zero bar, or (exact0: a mask) a non-zero entry
    where the stage writes exact zeros."""
    got = np.asarray(got, F64)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bar)
    r = np.where(np.isfinite(got) & np.isfinite(r), r, np.inf)
    if exact0 is not None:
        r = np.where(exact0 & (got != 0), np.inf, r)
    return float(r.max()) if r.size else 0.0


def fma32(a, b, c):
    """fl32(a b + c) of fp32 operands (the product is exact in fp64)."""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def bf16_round(a):
    return ac.rb16(a).astype(F32)


def range_rows(i, s):
    return int(s) * i.R, min((int(s) + 1) * i.R, i.N)


def tn_groups(i, n_rows):
    """k_tn_split's column-sum chains of a range of n_rows rows: (chain of every row, number of chains)."""
    g8 = (np.arange(n_rows) % 32) // 8
    return (g8, 4) if i.wide else (g8 % 2, 2)


def sample_rows(i):
    """The rows stages 4 - 6 look at: all, or (sample) the first, the last and 512 seeded rows."""
    if not i.case.sample:
        return np.arange(i.N)
    r = np.random.default_rng(31).choice(i.N, 512, replace=False)
    return np.unique(np.concatenate([[0, i.N - 1], r]))


def sample_ranges(i):
    """The row ranges stage 7 looks at: all, or (sample) the first, the last and six seeded ranges."""
    if not i.case.sample:
        return np.arange(i.S)
    r = np.random.default_rng(32).choice(np.arange(1, i.S - 1), 6, replace=False)
    return np.unique(np.concatenate([[0, i.S - 1], r]))


def bag_tiles(i, rows):
    """(bag, 32-row tile of the bag) pairs that hold the given batch rows."""
    b = i.bag_of[rows]
    return sorted(set(zip(b.tolist(), ((rows - i.off[b]) // 32).tolist())))


# ---- the stages: check_N(i, d) -> {name: error / bar};  emu_N(i, d, mut) fills d with the fp32 restatement -------------------------
# d: dict of the device's (or the restatement's) values — gB [nb, C, Kv], Dv [nb, C], qmax / gq [nb, C, 128], gA / gs [N, C],
# gz2 / H / Q / gH [N, 128], gqp: list per bag of [tiles, C, 128], part0 [S, 128, K], part1 [S, 128, 128], pb0 / pb1 [S, 128],
# part [splits, C, K], part_b [splits, C], g_<tensor>: the call's outputs.
def _p64(i, k):
    return np.asarray(i.w[k], F64)


def check_1(i, d):
    fw, out = _p64(i, "fcc_w"), {}
    r_gB, r_D = [], []
    for b in range(i.nb):
        t = i.g_pred[b].astype(F64)[:, None, None] * fw                                  # [o, c, k]
        P = i.g_B[b].astype(F64)[None] + np.cumsum(t, axis=0)
        r_gB.append(ratio(d["gB"][b], P[-1], 1.01 * LAM * U * np.sqrt((P ** 2).sum(axis=0))))
        sl = slice(int(i.off[b]), int(i.off[b + 1]))
        for c in range(i.C):
            t1 = d["gB"][b, c].astype(F64) * i.B[b, c].astype(F64)
            t2 = i.A[sl, c].astype(F64) * i.g_A[sl, c].astype(F64)
            ref, r2 = 0.0, 0.0
            part = np.zeros(256)
            for t12 in (t1, t2):                              # thread t: k = t, t + 256, ..; then n = t, t + 256, ..
                n = len(t12)
                pad = np.zeros(-(-n // 256) * 256)
                pad[:n] = t12
                pre = part[None] + np.cumsum(pad.reshape(-1, 256), axis=0)
                live = (np.arange(len(pad)) < n).reshape(-1, 256)
                r2 += ((pre * live) ** 2).sum()
                part = pre[-1]
            ref = part.sum()
            r2 += 8 * np.abs(part).sum() ** 2
            r_D.append(ratio(d["Dv"][b, c], ref, 1.01 * LAM * U * np.sqrt(r2)))
    out["gB"], out["D"] = max(r_gB), max(r_D)
    t = i.g_pred.astype(F64)[:, :, None, None] * i.B.astype(F64)[:, None]                # [b, o, c, k]
    if i.one:
        out["g_fcc_w"] = ratio(d["g_fcc_w"], t[0], 1.01 * U * np.abs(t[0]))
        out["g_fcc_b"] = 0.0 if np.array_equal(np.asarray(d["g_fcc_b"], F32).reshape(-1), i.g_pred[0]) else np.inf
    else:
        P = np.cumsum(t, axis=0)
        out["g_fcc_w"] = ratio(d["g_fcc_w"], P[-1], 1.01 * LAM * U * np.sqrt((P[1:] ** 2).sum(axis=0) + (t ** 2).sum(axis=0)))
        Pb = np.cumsum(i.g_pred.astype(F64), axis=0)
        out["g_fcc_b"] = ratio(d["g_fcc_b"], Pb[-1], 1.01 * LAM * U * np.sqrt((Pb[1:] ** 2).sum(axis=0)))
    return out


def emu_1(i, d, mut=None):
    fw = np.asarray(i.w["fcc_w"], F32)
    d["gB"] = np.zeros((i.nb, i.C, i.vals.shape[1]), F32)
    d["Dv"] = np.zeros((i.nb, i.C), F32)
    for b in range(i.nb):
        g = i.g_B[b].copy()
        for o in range(i.C):
            g = fma32(i.g_pred[b, o], fw[o], g)
        d["gB"][b] = g
        sl = slice(int(i.off[b]), int(i.off[b + 1]))
        for c in range(i.C):
            terms = [g[c] * i.B[b, c]] + ([] if mut == "D_without_AgA" else [i.A[sl, c] * i.g_A[sl, c]])
            part = np.zeros(256, F32)
            for t12 in terms:
                pad = np.zeros(-(-len(t12) // 256) * 256, F32)
                pad[:len(t12)] = t12
                for row in pad.reshape(-1, 256):
                    part = part + row
            while len(part) > 1:
                part = part[0::2] + part[1::2]
            d["Dv"][b, c] = part[0]
    t = i.g_pred[:, :, None, None] * i.B[:, None]
    d["g_fcc_w"] = np.cumsum(t, axis=0, dtype=F32)[-1]
    d["g_fcc_b"] = np.cumsum(i.g_pred, axis=0, dtype=F32)[-1]


def check_2(i, d):
    r = []
    for b in range(i.nb):
        sl = slice(int(i.off[b]), int(i.off[b + 1]))
        ref, bar = classes_bar(i.vals[sl], {"fc_w": d["gB"][b], "fc_b": np.zeros(i.C, F32)})
        r.append(ratio(d["gA"][sl], ref, bar))
    return {"gA": max(r)}


def emu_2(i, d, mut=None):
    d["gA"] = np.concatenate([i.vals[int(i.off[b]):int(i.off[b + 1])] @ d["gB"][b].T for b in range(i.nb)]).astype(F32)


def check_3(i, d):
    W1, b1 = _p64(i, "q0_w"), _p64(i, "q0_b")
    W2, b2 = (_p64(i, "q2_w"), _p64(i, "q2_b")) if i.nonlinear else (np.zeros((QD, QD)), np.zeros(QD))
    r = []
    for b in range(i.nb):
        xm = i.x[i.crit[b]].astype(F64)
        pre = xm @ W1.T + b1
        Hm = np.maximum(pre, 0) if i.nonlinear else pre
        rq_H2, rq_z2 = qmax_rand2(xm, Hm, W1, b1, W2, b2)
        if not i.nonlinear:
            r.append(ratio(d["qmax"][b], pre, 1.01 * LAM * np.sqrt(rq_H2)))
            continue
        q = np.tanh(Hm @ W2.T + b2)
        passes = pre > -LAM * np.sqrt(rq_H2)
        rz2 = (rq_H2 * passes) @ (W2 ** 2).T + rq_z2
        r.append(ratio(d["qmax"][b], q, 1.01 * (LAM * (1 - q * q) * np.sqrt(rz2) + 4 * U * np.abs(q))))
    return {"qmax": max(r)}


def emu_3(i, d, mut=None):
    p = {k: np.asarray(v, F32) for k, v in i.w.items()}
    h = i.x[i.crit.reshape(-1)] @ p["q0_w"].T + p["q0_b"]
    q = np.tanh(np.maximum(h, F32(0)) @ p["q2_w"].T + p["q2_b"]) if i.nonlinear else h
    d["qmax"] = q.astype(F32).reshape(i.nb, i.C, QD)


def check_4a(i, d, rows=None):
    rows = sample_rows(i) if rows is None else rows
    x = i.x[rows]
    pre, det, r2 = plane_ref(x, i.w["q0_w"], after=i.w["q0_b"])
    bar1 = plane_bar(det, r2)
    if not i.nonlinear:
        return {"Q": ratio(d["Q"][rows], pre, bar1)}
    out = {"H": ratio(d["H"][rows], np.maximum(pre, 0), bar1)}
    z, det, r2 = plane_ref(d["H"][rows], i.w["q2_w"], after=i.w["q2_b"])
    q = np.tanh(z)
    b_tanh = U * ((2 * np.abs(z) + 1) * (1 - q * q) + 3 * (1 - q) + 1)
    out["Q"] = ratio(d["Q"][rows], q, 1.01 * ((1 - q * q) * (det + LAM * np.sqrt(r2)) + b_tanh))
    return out


def emu_4a(i, d, mut=None, **kw):
    """mut: ("layer1" | "layer2", mm6 keywords)"""
    k1 = dict(kw, **(mut[1] if mut and mut[0] == "layer1" else {}))
    k2 = dict(kw, **(mut[1] if mut and mut[0] == "layer2" else {}))
    pre = mm6(i.x, i.w["q0_w"], **k1) + np.asarray(i.w["q0_b"], F32)
    if not i.nonlinear:
        d["Q"] = pre
        return
    if not (mut and mut[0] == "layer2"):
        d["H"] = np.maximum(pre, F32(0))
    if not (mut and mut[0] == "layer1"):
        d["Q"] = fast_tanh32(mm6(d["H"], i.w["q2_w"], **k2) + np.asarray(i.w["q2_b"], F32))


def _gs_terms(i, d):
    ga = d["gA"].astype(F64) + i.g_A.astype(F64)
    dd = ga - d["Dv"].astype(F64)[i.bag_of]
    return ga, dd


def check_4b(i, d, rows=None):
    rows = sample_rows(i) if rows is None else rows
    ga, dd = _gs_terms(i, d)
    A = i.A.astype(F64)
    ref = A * dd * SCALE32
    out = {"gs": ratio(d["gs"], ref, 1.01 * U * (np.abs(A) * SCALE32 * (np.abs(ga) + np.abs(dd)) + 2 * np.abs(ref)))}
    r = []
    for b, t in bag_tiles(i, rows):
        r0 = int(i.off[b]) + 32 * t
        r1 = min(r0 + 32, int(i.off[b + 1]))
        v = np.zeros((32, i.C, QD))
        v[:r1 - r0] = d["gs"][r0:r1].astype(F64)[:, :, None] * d["Q"][r0:r1].astype(F64)[:, None, :]
        r2 = (v ** 2).sum(axis=0) + halving_rand2(v)
        r.append(ratio(d["gqp"][b][t], v.sum(axis=0), 1.01 * LAM * U * np.sqrt(r2)))
    out["gqp"] = max(r)
    return out


def emu_4b(i, d, mut=None):
    ga = d["gA"] + i.g_A
    d["gs"] = (i.A * (ga - d["Dv"][i.bag_of]) * F32(SCALE32)).astype(F32)
    d["gqp"] = []
    for b in range(i.nb):
        n = i.lengths[b]
        T = -(-n // 32)
        v = np.zeros((T * 32, i.C, QD), F32)
        sl = slice(int(i.off[b]), int(i.off[b + 1]))
        v[:n] = d["gs"][sl][:, :, None] * d["Q"][sl][:, None, :]
        v = v.reshape(T, 32, i.C, QD).transpose(1, 0, 2, 3)
        while len(v) > 1:
            v = v[:len(v) // 2] + v[len(v) // 2:]
        d["gqp"].append(v[0])


def check_5(i, d, rows=None):
    rows = sample_rows(i) if rows is None else rows
    r = []
    for b in range(i.nb):
        g = d["gqp"][b]
        ref, r2 = chains_rand2(g, np.arange(len(g)) % 8, 8)
        r.append(ratio(d["gq"][b], ref, 1.01 * LAM * U * np.sqrt(r2)))
    out = {"gq": max(r)}
    bag = i.bag_of[rows]
    q = d["Q"][rows].astype(F64)
    t = 1 - q * q if i.nonlinear else np.ones_like(q)
    dt = q * q + t if i.nonlinear else np.zeros_like(q)        # |error of t| / u
    P = np.cumsum(d["gs"][rows].astype(F64)[:, :, None] * d["qmax"].astype(F64)[bag], axis=1)     # [n, C, 128]
    G = P[:, -1]
    ref = G * t
    bar = t * np.abs(P).sum(axis=1) + np.abs(G) * dt + (np.abs(ref) if i.nonlinear else 0.0)
    pos = {int(r_): k for k, r_ in enumerate(rows)}
    for b in range(i.nb):
        for c in range(i.C):
            k = pos.get(int(i.crit[b, c]))
            if k is None:
                continue
            g = d["gq"][b, c].astype(F64)
            ref[k] = ref[k] + g * t[k]
            bar[k] = bar[k] + np.abs(g) * dt[k] + (np.abs(g * t[k]) if i.nonlinear else 0.0) + np.abs(ref[k])
    out["gz2"] = ratio(d["gz2"][rows], ref, 1.01 * U * bar)
    return out


def emu_5(i, d, mut=None):
    d["gq"] = np.stack([chains32(g, np.arange(len(g)) % 8, 8) for g in d["gqp"]])
    q = bf16_round(d["Q"]) if mut == "Q_bf16" else d["Q"]
    t = (F32(1) - q * q) if i.nonlinear else np.ones_like(q)
    G = np.zeros((i.N, QD), F32)
    for c in range(i.C):
        G = fma32(d["gs"][:, c:c + 1], d["qmax"][i.bag_of, c], G)
    gz = (G * t).astype(F32) if i.nonlinear else G
    if mut != "no_gq":
        for b in range(i.nb):
            for c in range(i.C):
                n = int(i.crit[b, c])
                gz[n] = gz[n] + d["gq"][b, c] * t[n]
    d["gz2"] = gz


def check_6(i, d, rows=None):
    rows = sample_rows(i) if rows is None else rows
    ref, det, r2 = plane_ref(d["gz2"][rows], np.ascontiguousarray(np.asarray(i.w["q2_w"], F32).T))
    dead = ~(d["H"][rows] > 0)
    return {"gH": ratio(d["gH"][rows], np.where(dead, 0.0, ref), plane_bar(det, r2), exact0=dead)}


def emu_6(i, d, mut=None, **kw):
    g = mm6(d["gz2"], np.ascontiguousarray(np.asarray(i.w["q2_w"], F32).T), **dict(kw, **(mut or {})))
    d["gH"] = np.where(d["H"] > 0, g, F32(0)).astype(F32)


def _tn_operands(i, d):
    return [("part0", "pb0", d["gH"] if i.nonlinear else d["gz2"], i.x)] + ([("part1", "pb1", d["gz2"], d["H"])] if i.nonlinear else [])


def check_7(i, d, ranges=None):
    ranges = sample_ranges(i) if ranges is None else ranges
    out = {}
    for pk, bk, A0, X in _tn_operands(i, d):
        rp, rb = [], []
        for s in ranges:
            r0, r1 = range_rows(i, s)
            a, x = np.ascontiguousarray(A0[r0:r1].T), np.ascontiguousarray(X[r0:r1].T)
            ref, det, r2 = plane_ref(a, x)
            rp.append(ratio(d[pk][s], ref, plane_bar(det, r2)))
            grp, ng = tn_groups(i, r1 - r0)
            ref, r2 = chains_rand2(A0[r0:r1], grp, ng)
            rb.append(ratio(d[bk][s], ref, 1.01 * LAM * U * np.sqrt(r2)))
        out[pk], out[bk] = max(rp), max(rb)
    return out


def emu_7(i, d, mut=None, **kw):
    """mut: (partial's name, mm6 keywords)"""
    for pk, bk, A0, X in _tn_operands(i, d):
        k = dict(kw, **(mut[1] if mut and mut[0] == pk else {}))
        if mut and mut[0] != pk:
            continue
        d[pk] = np.stack([mm6(A0[r0:r1].T, X[r0:r1].T, **k) for r0, r1 in (range_rows(i, s) for s in range(i.S))])
        d[bk] = np.stack([chains32(A0[r0:r1], *tn_groups(i, r1 - r0)) for r0, r1 in (range_rows(i, s) for s in range(i.S))])


def _seq_bar(parts):
    P = np.cumsum(np.asarray(parts, F64), axis=0)
    return P[-1], 1.01 * LAM * U * np.sqrt((P ** 2).sum(axis=0))


def _small_range(i, s):
    return s * i.small_rows, min((s + 1) * i.small_rows, i.N)


def check_8(i, d):
    out = {}
    for gk, pk in (("g_q0_w", "part0"), ("g_q0_b", "pb0")) + ((("g_q2_w", "part1"), ("g_q2_b", "pb1")) if i.nonlinear else ()):
        ref, bar = _seq_bar(d[pk])
        out[gk] = ratio(d[gk], ref, bar)
    gc = i.g_classes.astype(F64)
    rp, rb = [], []
    for s in range(i.splits):
        r0, r1 = _small_range(i, s)
        grp = np.arange(r1 - r0) % 4
        ref, r2 = chains_rand2(gc[r0:r1, :, None] * i.x[r0:r1].astype(F64)[:, None, :], grp, 4, products=True)
        rp.append(ratio(d["part"][s], ref, 1.01 * LAM * U * np.sqrt(r2)))
        ref, r2 = chains_rand2(gc[r0:r1], grp, 4)
        rb.append(ratio(d["part_b"][s], ref, 1.01 * LAM * U * np.sqrt(r2)))
    out["part"], out["part_b"] = max(rp), max(rb)
    # the sums over the ranges, then the sparse max-stream term bag by bag
    for gk, pk, sparse in (("g_fc_w", "part", i.g_max.astype(F64)[:, :, None] * i.x[i.crit].astype(F64)),
                           ("g_fc_b", "part_b", i.g_max.astype(F64))):
        ref, bar = _seq_bar(d[pk])
        for b in range(i.nb):
            ref = ref + sparse[b]
            bar = bar + 1.01 * U * (np.abs(sparse[b]) + np.abs(ref))
        out[gk] = ratio(d[gk], ref, bar)
    return out


def emu_8(i, d, mut=None):
    for gk, pk in (("g_q0_w", "part0"), ("g_q0_b", "pb0")) + ((("g_q2_w", "part1"), ("g_q2_b", "pb1")) if i.nonlinear else ()):
        d[gk] = np.cumsum(d[pk], axis=0, dtype=F32)[-1]
    part, part_b = [], []
    for s in range(i.splits):
        r0, r1 = _small_range(i, s)
        grp = np.arange(r1 - r0) % 4
        part.append(chains32(i.g_classes[r0:r1, :, None] * i.x[r0:r1][:, None, :], grp, 4))
        part_b.append(chains32(i.g_classes[r0:r1], grp, 4))
    d["part"], d["part_b"] = np.stack(part), np.stack(part_b)
    gw, gb = np.cumsum(d["part"], axis=0, dtype=F32)[-1], np.cumsum(d["part_b"], axis=0, dtype=F32)[-1]
    for b in range(i.nb):
        gw = gw + i.g_max[b][:, None] * i.x[i.crit[b]]
        gb = gb + i.g_max[b]
    d["g_fc_w"], d["g_fc_b"] = gw.astype(F32), gb.astype(F32)


def check_9(i, d):
    t = i.A.astype(F64)[:, :, None] * d["gB"].astype(F64)[i.bag_of]           # [N, C, Kv]
    P = np.cumsum(t, axis=1)
    return {"g_vals": ratio(d["g_vals"], P[:, -1], 1.01 * U * (np.abs(P).sum(axis=1) + np.abs(t).sum(axis=1)))}


def emu_9(i, d, mut=None):
    acc = np.zeros((i.N, d["gB"].shape[2]), F32)
    for c in range(i.C):
        acc = fma32(i.A[:, c:c + 1], d["gB"][i.bag_of, c], acc)
    d["g_vals"] = acc


def check_10(i, d):
    Lm = d["gH"] if i.nonlinear else d["gz2"]
    ref, det, r2 = plane_ref(Lm, np.ascontiguousarray(np.asarray(i.w["q0_w"], F32).T))
    Wf = _p64(i, "fc_w")
    is_crit = np.zeros((i.N, i.C), bool)
    gm = np.zeros((i.N, i.C))
    for b in range(i.nb):
        for c in range(i.C):
            is_crit[i.crit[b, c], c] = True
            gm[i.crit[b, c], c] = i.g_max[b, c]
    cf = i.g_classes.astype(F64) + gm
    lin = np.zeros_like(ref)
    for c in range(i.C):
        lin = lin + U * (np.abs(cf[:, c]) * is_crit[:, c])[:, None] * np.abs(Wf[c])[None]       # the rounding of g_classes + g_max
        ref = ref + cf[:, c:c + 1] * Wf[c][None]
        r2 = r2 + U * U * ref ** 2
        if i.identity_v:
            ref = ref + i.A[:, c:c + 1].astype(F64) * d["gB"].astype(F64)[i.bag_of, c]
            r2 = r2 + U * U * ref ** 2
    return {"g_feats": ratio(d["g_feats"], ref, 1.01 * (det + lin + LAM * np.sqrt(r2)))}


def emu_10(i, d, mut=None, **kw):
    Lm = d["gH"] if i.nonlinear else d["gz2"]
    v = mm6(Lm, np.ascontiguousarray(np.asarray(i.w["q0_w"], F32).T), **dict(kw, **(mut or {})))
    cf = i.g_classes.copy()
    for b in range(i.nb):
        for c in range(i.C):
            cf[i.crit[b, c], c] += i.g_max[b, c]
    Wf = np.asarray(i.w["fc_w"], F32)
    for c in range(i.C):
        v = fma32(cf[:, c:c + 1], Wf[c][None], v)
        if i.identity_v:
            v = fma32(i.A[:, c:c + 1], d["gB"][i.bag_of, c], v)
    d["g_feats"] = v


CHECKS = {"1": check_1, "2": check_2, "3": check_3, "4a": check_4a, "4b": check_4b, "5": check_5, "6": check_6, "7": check_7,
          "8": check_8, "9": check_9, "10": check_10}
EMUS = {"1": emu_1, "2": emu_2, "3": emu_3, "4a": emu_4a, "4b": emu_4b, "5": emu_5, "6": emu_6, "7": emu_7, "8": emu_8,
        "9": emu_9, "10": emu_10}
PLANE_STAGES = ("4a", "6", "7", "10")


def case_stages(c):
    """The stages a case checks (the docstring of tests/test_agg_bwd_precision_gpu.py says which case is there for what)."""
    st = [s for s in STAGES if s not in ("6", "9", "10")]
    if c.nonlinear:
        st.append("6")
    if c.own_vals:
        st.append("9")
    if c.gx:
        st.append("10")
    return sorted(st, key=STAGES.index)


def emulate(i, plain=False):
    """Every stage of the case restated in fp32 numpy, each fed with the restatement's own earlier stages: the `d` of the checks."""
    d = {}
    for st in case_stages(i.case):
        if st in PLANE_STAGES:
            EMUS[st](i, d, plain=plain)
        else:
            EMUS[st](i, d)
    return d


def check_all(i, d):
    """{stage: {name: error / bar}} for the stages of the case."""
    return {st: CHECKS[st](i, d) for st in case_stages(i.case)}


def host_inputs(c):
    """The inputs of a case with the forward's outputs restated in fp32 numpy (no GPU), and the layout from the library's query."""
    import dsmil_wsi_amd._native as nat
    x, lengths = case_rows(c.name)
    w = case_weights(c)
    off = np.concatenate([[0], np.cumsum(lengths)])
    vals = x if not c.own_vals else case_vals(c.name)
    outs = [forward32(x[off[b]:off[b + 1]], w, c.nonlinear) for b in range(len(lengths))]
    A = np.concatenate([o[0] for o in outs])
    B = np.stack([(o[0].T @ vals[off[b]:off[b + 1]]).astype(F32) for b, o in enumerate(outs)])
    idx = np.stack([o[2] for o in outs])
    K, C = ac.dims(c.s)
    lay = nat.backward_layout(0 if c.entry == "one" else len(lengths), len(x), K, K, C, int(c.nonlinear), int(not c.misalign), 1)
    return build_inputs(c, A, B, idx, lay), lay
