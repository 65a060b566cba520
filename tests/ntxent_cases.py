"""Cases, the fp64 closed form, a numpy emulation of the kernels' arithmetic and DERIVED bars of the native NT-Xent loss
(csrc/ntxent.hip behind ops.ntxent_forward / ntxent_backward and simclr.NTXentLoss), shared by tests/test_ntxent_host.py and
tests/test_ntxent_gpu.py.  Nothing here is tuned on a GPU or taken from the code under test; the reference is `closed_form`
below in fp64, which tests/test_ntxent_host.py holds to the reference class's own fp64 values (tests/golden/ntxent_golden.npz).

R = cat([zjs, zis]), M = 2N, p(a) = (a + N) mod M, x = R^ (cosine: rows over max(norm, 1e-8)) or R (dot), z = x x^T / T:
    loss = (1/M) sum_a (lse_a - z_{a,p(a)}),  lse_a = logsumexp_{b != a} z_ab
    P_ab = exp(z_ab - lse_a) (P_aa = 0),  Wn = (P + P^T - 2 Pi) / M,  d^ = Wn x / T,  g_a = (d^_a - x_a (x_a . d^_a)) / |R_a|

u = 2^-24.  Errors are of two kinds, as in tests/agg_precision_cases.py: det (a fixed function of the data, possibly one-sided:
worst case, formed with its signs where both factors are known here) and rand (fp32 roundings, each at most u x |the value
rounded|, independent: n of them enter as LAM sqrt(sum (coefficient b_i)^2), LAM = 4).  1.01 pays for second order.

LOGITS.  Operand: x' = fl(x_fp32 f) 2^e with f = fl(1 / max(fl(sqrt(ss)), 1e-8)); h0 = rne16(x'), h1 = rne16(x' - h0).
  row norm   ss by one fma chain of ceil(D / 64) per lane and six exchange levels, partial sums below ss; sqrt halves the
             relative error; sqrt and the division round once each:  delta_a = sum of independent errors with
             q_n = u^2 ((ceil(D / 64) + 6) / 4 + 2) (relative).  It is shared by row a's logits (enters with its sign, bound
             dn = LAM sqrt(q_n)) and independent from row to row (quadrature over b).
  element    x' = fl(x f): u relative per element, independent: u^2 sum_k 2 (x_ak x_bk)^2 on S_ab.
  planes     r = x' - h0 - h1 and the dropped product h1 h1 are FORMED from the same cut in numpy:
             det_S[a, b] = | sum_k r_ak x_bk + x_ak r_bk + h1_ak h1_bk |  (unscaled units).
  MFMA       three plane products per 32-k window into one fp32 accumulator (v_mfma_f32_16x16x32_f16), at most one rounding
             per product added, windows in k order; with Pk the fp64 prefix at the window borders and S_s = sum |x||x|:
             rand_S^2 = u^2 32 sum_s ((|Pk_(s-1)| + S_s)^2 + 2 (max(|Pk_(s-1)|, |Pk_s|) + S_s / 64)^2)   (tests/agg_precision_cases.py)
  1 / T      the kernel gets fl32(T), forms fl(1 / T) and one product: 3 u |z_ab| (det).
  z_ab and z_ba are the same sums in the same order: ONE error per unordered pair.
LSE.  Each exp is exp2(fl(d log2e)) on the hardware: the subtraction, the constant and the product 3 u |d| on the exponent,
  v_exp_f32 1 ulp: (3 |d| + 2) u relative, d = z_ab - (row maximum): the online rescales telescope, the differences all of one
  sign, so |d| is the whole distance; nfac = (tiles per split) + 3 rescale factors of (2 + 1) u; 16 (tiles per split) + 2 +
  (splits) additions below l; logf 1 ulp, the final addition:
      B_lse[a] = u (sum_b P_ab (3 |z_ab - zmax_a| + 2) + 3 nfac + LAM sqrt(nadd) + 2 |log l_a| + |lse_a|)       (det)
LOSS = sum_ab G_ab dz_ab + mean_a eps_lse + the final sum (rows by 1024 chains, ten tree levels, the division):
      bar_loss = 1.01 (sum |G| det_z + dn-term in quadrature over rows + mean B_lse + LAM sqrt(pairs (G_ab + G_ba)^2 rand_z^2)
                       + u (LAM sqrt(ceil(M / 1024) + 10) + 2) mean |lse_a - z_ap| )
GRADIENT.  To first order, with dz symmetric and Q = P + P^T, mu_a = sum_b P_ab x_b:
      M T dd^_ak = sum_b dz_ab (Q_ab x_bk - P_ab mu_ak)  -  sum_b P_ba x_bk (sum_d P_bd dz_bd)  + (errors of W, of GEMM 2)
  row a's own logits: rand in quadrature over b, det with absolute values, the shared delta_a with its sign;
  the other rows' normalisers: Ebar_b = sum_d P_bd det_bd + LAM sqrt(sum_d P_bd^2 rand_bd^2), then sum_b P_ba |x_bk| Ebar_b;
  W: P_ab carries (3 |z_ab - lse_a| + 2) u + B_lse[a] relative (the backward's exp, the forward's lse), two additions 2 u |W|;
  W's planes (cut from the kernel's own value, so bounded): 2 u |W| + 2^-36 residue, the dropped product 2^-11 (1 + 2^-10) |W|
  |h1|; x's residue against the known Wn is formed; x_b's own delta_b: q_n sum_b (Wn_ab x_bk)^2;
  GEMM 2: as rand_S over 32-b windows, the prefix restarting at every column split (nx_plan's geometry, restated in `plan`),
  then the splits added in order: u^2 sum (prefix of the partials)^2;
  epilogue: three factors 3 u |d^|; the projection's dot by ceil(D / 64) fmas per lane and six levels; the products:
      epi = u (3 |d^_ak| + |x_ak| (LAM sqrt(ceil(D / 64) + 6) sum_j |x_aj d^_aj| + 2 |x_a . d^_a|) + 2 |pr_ak|)
  and an error e of d^ reaches g through the projection: |e_ak| + |x_ak| sum_j |x_aj| |e_aj|, all times 1 / |R_a|; delta_a
  itself dn |g_ak|."""
import functools

import numpy as np

U = 2.0 ** -24
LAM = 4.0
LOG2E32 = np.float32(1.44269504088896341)

# (N, D, T, cosine) — the table of the issue, in its order
CASES = [(1, 8, .5, 1), (2, 8, .5, 1), (33, 256, .5, 1), (64, 256, .5, 1), (65, 100, .1, 1), (40, 512, .05, 1),
         (300, 128, .5, 1), (1030, 64, .5, 1), (17, 64, .5, 0), (96, 256, .2, 0)]
# the cases small enough for the committed golden file (the reference class forms [2N, 2N, D] in fp64)
GOLDEN_CASES = [(1, 8, .5, 1), (2, 8, .5, 1), (33, 256, .5, 1), (65, 100, .1, 1), (17, 64, .5, 0),
                (20, 48, .5, 1, "spread")]


def case_name(c):
    return "N%d_D%d_T%g_%s%s" % (c[0], c[1], c[2], "cos" if c[3] else "dot", "_" + c[4] if len(c) > 4 else "")


@functools.lru_cache(maxsize=None)
def make_inputs(case):
    """(zis, zjs) fp32 [N, D]: two correlated views (correlation min(0.9, 5 T)).  Cosine cases: rows of norm about 1; dot cases: unnormalised rows of
    scale 0.5 (norm about 0.5); flavour "spread": row norms 10^U(-3, 3); "twins": zis == zjs and samples 0 and 1 identical."""
    N, D = case[0], case[1]
    flavour = case[4] if len(case) > 4 else ""
    rng = np.random.default_rng(9000 + 7 * N + D + (0 if case[3] else 1))
    a = rng.normal(0, 1, (N, D))
    c = min(0.9, 5 * case[2])          # cosine of a positive pair: its logit stays near the negatives' log-sum-exp, so a sharp
    b = c * a + np.sqrt(1 - c * c) * rng.normal(0, 1, (N, D))      # softmax (small T) is not a saturated one
    s = (1.0 if case[3] else 0.5) / np.sqrt(D)
    a, b = a * s, b * s
    if flavour == "spread":
        a = a * 10 ** rng.uniform(-3, 3, (N, 1))
        b = b * 10 ** rng.uniform(-3, 3, (N, 1))
    if flavour == "twins":
        a[1] = a[0]
        b = a.copy()
    zis, zjs = a.astype(np.float32), b.astype(np.float32)
    zis.setflags(write=False)
    zjs.setflags(write=False)
    return zis, zjs


def closed_form(zis, zjs, T, cosine, full=False):
    """fp64: (loss, g_zis, g_zjs) [, dict of the intermediate quantities the bars use]."""
    R = np.concatenate([np.asarray(zjs, np.float64), np.asarray(zis, np.float64)], 0)
    M, N = R.shape[0], R.shape[0] // 2
    nrm = np.maximum(np.sqrt((R * R).sum(1, keepdims=True)), 1e-8) if cosine else np.ones((M, 1))
    x = R / nrm
    z = x @ x.T / T
    idx = np.arange(M)
    pa = (idx + N) % M
    zm = z.copy()
    zm[idx, idx] = -np.inf
    zmax = zm.max(1, keepdims=True)
    ex = np.exp(zm - zmax)
    l = ex.sum(1, keepdims=True)
    lse = (zmax + np.log(l))[:, 0]
    pos = z[idx, pa]
    loss = float(np.mean(lse - pos))
    P = ex / l
    Pi = np.zeros((M, M))
    Pi[idx, pa] = 1.0
    Wn = (P + P.T - 2 * Pi) / M
    dh = Wn @ x / T
    dot = (x * dh).sum(1, keepdims=True)
    g = (dh - x * dot) / nrm if cosine else dh
    out = (loss, g[N:].copy(), g[:N].copy())
    if not full:
        return out
    return out + (dict(R=R, x=x, nrm=nrm, z=z, zmax=zmax[:, 0], l=l[:, 0], lse=lse, pos=pos, P=P, Pi=Pi, Wn=Wn, dh=dh, dot=dot,
                       g=g, M=M, N=N),)


def plan(N, D):
    """nx_plan of csrc/ntxent.hip: (Mpad, Dpad, forward splits, tiles per split, backward splits, tiles per split)."""
    M = 2 * N
    Mpad, Dpad = (M + 63) // 64 * 64, (D + 31) // 32 * 32
    rb, nfc = Mpad // 64, (Dpad + 255) // 256

    def split(want):
        want = min(max(want, 1), 8, rb)
        tps = (rb + want - 1) // want
        return (rb + tps - 1) // tps, tps
    return (Mpad, Dpad) + split((512 + rb - 1) // rb) + split((256 + rb * nfc - 1) // (rb * nfc))


def workspace_bound(N, D):
    """16 M Dpad 4 + 1 MiB: the O(M D) ceiling of the issue."""
    return 16 * 2 * N * ((D + 31) // 32 * 32) * 4 + (1 << 20)


# ------------------------------------------------------------------------------------------------ the operand cut, shared
def _f32(a):
    return np.asarray(a, np.float32)


def _lane_sum(terms):
    """fp32: lane (k mod 64) adds its terms in sequence (an fma per term), then six exchange levels.  terms [rows, D] fp64
    (exact products of fp32 values)."""
    rows, D = terms.shape
    nch = (D + 63) // 64
    t = np.zeros((rows, nch * 64))
    t[:, :D] = terms
    t = t.reshape(rows, nch, 64)
    acc = np.zeros((rows, 64), np.float32)
    for c in range(nch):
        acc = (acc.astype(np.float64) + t[:, c]).astype(np.float32)
    off = 32
    while off >= 1:
        acc = acc + acc[:, np.arange(64) ^ off]
        off >>= 1
    return acc[:, 0]


def operand(zis, zjs, cosine, planes=2):
    """The kernels' operand: (R fp32 [M, D], inv fp32 [M], e, h0, h1 [M, Dpad] as fp64 in scaled units, xk = fl(R inv) as fp64).
    planes = 1 drops h1 (the degraded variant of the host test)."""
    R = np.concatenate([_f32(zjs), _f32(zis)], 0)
    M, D = R.shape
    Dpad = (D + 31) // 32 * 32
    R64 = R.astype(np.float64)
    if cosine:
        ss = _lane_sum(R64 * R64)
        inv = np.float32(1.0) / np.maximum(np.sqrt(ss).astype(np.float32), np.float32(1e-8))
        e = 13
    else:
        inv = np.ones(M, np.float32)
        mx = float(np.abs(R).max())
        e = 14 - int(np.frexp(mx)[1]) if mx > 0 else 0
    f = (inv.astype(np.float64) * 2.0 ** e).astype(np.float32)            # exact
    xs = np.zeros((M, Dpad), np.float32)
    xs[:, :D] = R * f[:, None]                                            # one fp32 rounding
    h0 = xs.astype(np.float16)
    h1 = (xs - h0.astype(np.float32)).astype(np.float16)
    if planes == 1:
        h1 = np.zeros_like(h1)
    return R, inv, e, h0.astype(np.float64), h1.astype(np.float64), xs.astype(np.float64)


def _mfma_gemm(A0, A1, B0, B1, acc=None):
    """fp32 accumulator over 32-k windows, three plane products per window, smallest first; one rounding per product and window
    (the least an MFMA may do).  A* [m, K], B* [n, K] -> [m, n] fp32."""
    K = A0.shape[1]
    if acc is None:
        acc = np.zeros((A0.shape[0], B0.shape[0]), np.float32)
    for k0 in range(0, K, 32):
        s = slice(k0, k0 + 32)
        for (a, b) in ((A1, B0), (A0, B1), (A0, B0)):
            acc = (acc.astype(np.float64) + a[:, s] @ b[:, s].T).astype(np.float32)
    return acc


def _exp32(d):
    return np.exp2((_f32(d) * LOG2E32).astype(np.float64)).astype(np.float32)


def emulate(zis, zjs, T, cosine, planes=2, g_loss=1.0):
    """The kernels' arithmetic in numpy: (loss fp32, g_zis, g_zjs fp32, lse fp32)."""
    R, inv, e, h0, h1, _ = operand(zis, zjs, cosine, planes)
    M, D = R.shape
    N = M // 2
    Mpad, Dpad, nsf, tpf, nsb, tpb = plan(N, D)
    H0, H1 = np.zeros((Mpad, Dpad)), np.zeros((Mpad, Dpad))
    H0[:M], H1[:M] = h0, h1
    isc = np.float32(2.0 ** -e)
    cz = np.float32(isc * (np.float32(1.0) / np.float32(T)))
    S = _mfma_gemm(H0[:M], H1[:M], H0, H1)                                # [M, Mpad]
    v = (S * isc) * cz
    idx = np.arange(M)
    pa = (idx + N) % M
    pos = v[idx, pa]
    NEG = np.float32(-3.0e38)
    valid = (np.arange(Mpad)[None, :] < M) & (np.arange(Mpad)[None, :] != idx[:, None])
    vm = np.where(valid, v, NEG).astype(np.float32)
    # lane (a, g) holds b = 64 t + 16 bb + 4 g + e of tile t, in the order (bb, e)
    nt = Mpad // 64
    lanes = vm.reshape(M, nt, 4, 4, 4).transpose(0, 3, 1, 2, 4).reshape(M, 4, nt, 16)
    pm, pl = [], []
    with np.errstate(over="ignore", under="ignore"):
        for s in range(nsf):
            m = np.full((M, 4), NEG, np.float32)
            l = np.zeros((M, 4), np.float32)
            for t in range(s * tpf, min(nt, (s + 1) * tpf)):
                tv = lanes[:, :, t]
                tmax = tv.max(2)
                mn = np.maximum(m, tmax)
                ln = l * _exp32(m - mn)
                for i in range(16):
                    ln = np.where(tv[:, :, i] > NEG, ln + _exp32(tv[:, :, i] - mn), ln)
                upd = tmax > NEG
                l, m = np.where(upd, ln, l).astype(np.float32), np.where(upd, mn, m)
            for sel in ((0, 1, 2, 3), (0, 2)):                            # lanes g ^ 1, then g ^ 2
                if len(sel) == 4:
                    m2, l2 = m[:, [1, 0, 3, 2]], l[:, [1, 0, 3, 2]]
                else:
                    m2, l2 = m[:, [2, 3, 0, 1]], l[:, [2, 3, 0, 1]]
                mn = np.maximum(m, m2)
                x_, y_ = l * _exp32(m - mn), l2 * _exp32(m2 - mn)
                l, m = (x_ + y_).astype(np.float32), mn
            pm.append(m[:, 0])
            pl.append(l[:, 0])
        mfin = np.max(np.stack(pm), 0)
        lfin = np.zeros(M, np.float32)
        for s in range(nsf):
            lfin = lfin + pl[s] * _exp32(pm[s] - mfin)
    lse = (mfin + np.log(lfin.astype(np.float64)).astype(np.float32)).astype(np.float32)
    rowloss = (lse - pos).astype(np.float32)
    th = np.zeros(1024, np.float32)
    for a0 in range(0, M, 1024):
        seg = rowloss[a0:a0 + 1024]
        th[:len(seg)] += seg
    s_ = 512
    while s_ >= 1:
        th[:s_] = th[:s_] + th[s_:2 * s_]
        s_ >>= 1
    loss = np.float32(th[0] / np.float32(M))
    # backward
    lse_b = np.zeros(Mpad, np.float32)
    lse_b[:M] = lse
    with np.errstate(over="ignore", under="ignore"):
        W = (_exp32(v - lse[:, None]) + _exp32(v - lse_b[None, :])).astype(np.float32)
    W[idx, pa] = W[idx, pa] - np.float32(2.0)
    W = np.where(valid, W, np.float32(0)).astype(np.float32)
    Ws = W * np.float32(4096.0)
    w0 = Ws.astype(np.float16)
    w1 = (Ws - w0.astype(np.float32)).astype(np.float16)
    if planes == 1:
        w1 = np.zeros_like(w1)
    w0, w1 = w0.astype(np.float64), w1.astype(np.float64)
    parts = []
    for s in range(nsb):
        cs = slice(s * tpb * 64, min(Mpad, (s + 1) * tpb * 64))
        parts.append(_mfma_gemm(w0[:, cs], w1[:, cs], H0[cs].T, H1[cs].T))   # [M, Dpad]
    d = np.zeros((M, Dpad), np.float32)
    for p_ in parts:
        d = d + p_
    fac = np.float32(1.0 / (4096.0 * M * float(np.float32(T))))
    f = np.float32(np.float32(g_loss) * np.float32(fac * isc))
    d = (d[:, :D] * f).astype(np.float32)
    if cosine:
        r = (R * inv[:, None]).astype(np.float32)
        dot = _lane_sum(r.astype(np.float64) * d.astype(np.float64))
        g = ((d - r * dot[:, None]) * inv[:, None]).astype(np.float32)
    else:
        g = d
    return loss, g[N:], g[:N], lse


# ------------------------------------------------------------------------------------------------ the bars
def _window_rand2(A, B, win=32, restarts=None):
    """sum over windows of win ((|P_(s-1)| + S_s)^2 + 2 (max(|P_(s-1)|, |P_s|) + S_s / 64)^2) for the product A B^T summed
    over the shared axis (A [m, K], B [n, K]); the prefix restarts at the indices in `restarts`.  Also returns the list of
    the partial products between restarts (for the split sum)."""
    K = A.shape[1]
    restarts = set(restarts or ())
    P = np.zeros((A.shape[0], B.shape[0]))
    out = np.zeros_like(P)
    partials = []
    for k0 in range(0, K, win):
        if k0 in restarts and k0:
            partials.append(P)
            P = np.zeros_like(P)
        s = slice(k0, k0 + win)
        Pn = P + A[:, s] @ B[:, s].T
        Ss = np.abs(A[:, s]) @ np.abs(B[:, s]).T
        out += win * ((np.abs(P) + Ss) ** 2 + 2 * (np.maximum(np.abs(P), np.abs(Pn)) + Ss / 64) ** 2)
        P = Pn
    partials.append(P)
    return out, partials


@functools.lru_cache(maxsize=None)
def reference(case, g_loss=1.0):
    """(loss, g_zis, g_zjs, bar_loss, bar_g_zis, bar_g_zjs) for a case of make_inputs, fp64; the gradients and their bars are
    for the upstream gradient g_loss."""
    zis, zjs = make_inputs(case)
    return reference_of(zis, zjs, case[2], case[3], g_loss)


def reference_of(zis, zjs, T, cosine, g_loss=1.0):
    loss, g_zis, g_zjs, q = closed_form(zis, zjs, T, cosine, full=True)
    M, N, x, z, P, Wn, dh = q["M"], q["N"], q["x"], q["z"], q["P"], q["Wn"], q["dh"]
    D = x.shape[1]
    Mpad, Dpad, nsf, tpf, nsb, tpb = plan(N, D)
    nch = (D + 63) // 64
    q_n = U * U * ((nch + 6) / 4 + 2) if cosine else 0.0
    dn = LAM * np.sqrt(q_n)
    # the cut, formed from the kernel's own operand definition
    _, inv, e, h0, h1, xs = operand(zis, zjs, cosine)
    sc = 2.0 ** -e
    xk, h1u = xs * sc, h1 * sc                                       # the operand the kernel cuts, its low plane (unscaled)
    r = (xs - h0 - h1) * sc
    det_S = np.abs(r @ xk.T + xk @ r.T + h1u @ h1u.T)
    xp = np.zeros((M, Dpad))
    xp[:, :D] = x
    rand_S2 = U * U * (_window_rand2(xp, xp)[0] + 2 * (xp * xp) @ (xp * xp).T)
    det_z = det_S / T + 3 * U * np.abs(z)
    rand_z2 = rand_S2 / T ** 2                                        # per unordered pair
    off = ~np.eye(M, dtype=bool)
    det_z, rand_z2 = det_z * off, rand_z2 * off
    # lse
    nfac, nadd = tpf + 3, 16 * tpf + 2 + nsf
    dist = np.abs(z - q["zmax"][:, None]) * off
    B_lse = U * ((P * (3 * dist + 2)).sum(1) + 3 * nfac + LAM * np.sqrt(nadd) + 2 * np.abs(np.log(q["l"])) + np.abs(q["lse"]))
    # loss
    G = (P - q["Pi"]) / M
    Gs = G + G.T
    rowc = (Gs * z).sum(1)                                            # d loss / d delta_a
    rowl = np.abs(q["lse"] - q["pos"])
    bar_loss = 1.01 * ((np.abs(G) * det_z).sum() + LAM * np.sqrt(q_n * (rowc ** 2).sum()) + B_lse.mean()
                       + LAM * np.sqrt(0.5 * (Gs ** 2 * rand_z2).sum())
                       + U * (LAM * np.sqrt((M + 1023) // 1024 + 10) + 2) * rowl.mean()) + 1e-45
    # gradient: d^ first (times M T), then the projection
    Q = P + P.T
    mu = P @ x
    ax = np.abs(x)
    rz = rand_z2 + q_n * z * z * off                                  # the other row's normaliser, independent over b
    own_rand2 = (Q * Q * rz) @ (x * x) - 2 * mu * ((Q * P * rz) @ x) + mu * mu * (P * P * rz).sum(1, keepdims=True)
    own_rand2 = np.maximum(own_rand2, 0)
    own_det = (Q * det_z) @ ax + np.abs(mu) * (P * det_z).sum(1, keepdims=True)
    own_dn = dn * np.abs((Q * z * off) @ x - mu * (P * z * off).sum(1, keepdims=True))
    Ebar = (P * (det_z + dn * np.abs(z) * off)).sum(1) + LAM * np.sqrt((P * P * rz).sum(1))
    others = (P.T * Ebar[None, :]) @ ax
    rho = (3 * np.abs(z - q["lse"][:, None]) + 2) * U * off + B_lse[:, None]
    w_exp = (P * rho + (P * rho).T) @ ax + 2 * U * np.abs(M * Wn) @ ax
    aW = np.abs(M * Wn)
    w_planes = aW @ (2 * U * ax + 2.0 ** -11 * (1 + 2.0 ** -10) * np.abs(h1u[:, :D])) + np.abs((M * Wn) @ r[:, :D]) \
        + 2.0 ** -36 * np.ones((M, M)) @ ax
    x_dn2 = q_n * ((M * Wn) ** 2) @ (x * x)
    restarts = [s * tpb * 64 for s in range(1, nsb)]
    Wp = np.zeros((M, Mpad))
    Wp[:, :M] = M * Wn
    xT = np.zeros((D, Mpad))
    xT[:, :M] = x.T
    g2, partials = _window_rand2(Wp, xT, restarts=restarts)
    pref, split2 = np.zeros_like(partials[0]), np.zeros_like(partials[0])
    for p_ in partials[:-1] if len(partials) > 1 else []:
        pref = pref + p_
        split2 += (np.abs(pref) + 0) ** 2
    if len(partials) > 1:
        split2 += (M * T * dh) ** 2
    gemm2_rand2 = U * U * (g2 + split2)
    e_dh = (own_det + own_dn + others + w_exp + w_planes + LAM * np.sqrt(own_rand2 + x_dn2 + gemm2_rand2)) / (M * T)
    if cosine:
        epi = U * (3 * np.abs(dh) + ax * (LAM * np.sqrt(nch + 6) * (ax * np.abs(dh)).sum(1, keepdims=True) + 2 * np.abs(q["dot"]))
                   + 2 * np.abs(dh - x * q["dot"]))
        e_g = (e_dh + ax * (ax * e_dh).sum(1, keepdims=True) + epi) / q["nrm"] + (dn + 2 * U) * np.abs(q["g"])
    else:
        e_g = e_dh + 3 * U * np.abs(dh)
    bar_g = 1.01 * abs(g_loss) * (e_g + U * np.abs(q["g"])) + 1e-45
    return loss, g_loss * g_zis, g_loss * g_zjs, bar_loss, bar_g[N:], bar_g[:N]


def ratios(got, ref):
    """max |error| / bar of (loss, g_zis, g_zjs) against reference()'s tuple."""
    loss, g_zis, g_zjs = (np.asarray(t, np.float64) for t in got)
    return (float(abs(loss - ref[0]) / ref[3]), float(np.max(np.abs(g_zis - ref[1]) / ref[4])),
            float(np.max(np.abs(g_zjs - ref[2]) / ref[5])))
