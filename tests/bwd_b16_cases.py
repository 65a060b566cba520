"""Cases, seeded operands and the fp64 reference of the aggregator backward on bf16-stored rows, shared by
tests/test_bwd_b16_host.py (the formula is the gradient; the bar is reachable; the host deviation of check (g)) and
tests/test_bwd_b16_gpu.py (the kernels meet the bar).

The gradient under test is the analytic gradient in the header of csrc/agg_bwd.hip with x := the bf16 rows and W := the
bf16-rounded weights, fed the FORWARD'S OWN A, B and idx (straight-through for the forward's roundings)."""
import functools

import numpy as np
import torch

from inputs import make_bag
from util import GOLDEN_CLASSES, VARIANT, class_set_weights, load_weights

KEYS = ("fc_w", "fc_b", "q0_w", "q0_b", "q2_w", "q2_b", "fcc_w", "fcc_b")

# (tag, N): dense upstream gradients on pred, classes, A and B everywhere
CASES = [("tcga", 1),           # one-row bag
         ("tcga", 31),          # below one 32-row tile
         ("tcga", 33),          # partial second 32-row tile
         ("tcga", 64), ("tcga", 65),   # the 64-row hidden-split tile boundary
         ("tcga", 700),         # many tiles
         ("linq", 50),          # linear query
         ("tree", 300),         # K = 1024
         ("K64_C5_nl", 40),     # five classes, one feature chunk (weights of the classes golden file)
         ("tcga", 65664)]       # 513 x 128 rows: the four-wave regime
BATCH = [1, 2, 127, 128, 129, 31, 700]   # K = 512, C = 2 (tcga)
HOST_DEV_CASES = [("tcga", 33), ("tcga", 200), ("tcga", 700), ("linq", 50), ("tree", 300)]   # check (g)


def round_bf16(a):
    """fp32 array -> its bf16 rounding (torch's, round to nearest even) as fp32."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def variant(tag):
    """(K, C, nonlinear) of a weight set."""
    if tag == "K64_C5_nl":
        return 64, 5, True
    K, C, nonlinear, _ = VARIANT[tag]
    return K, C, bool(nonlinear)


@functools.lru_cache(maxsize=None)
def weights(tag):
    """The weight set `tag`, every tensor rounded to bf16 (what ops._bf16_params hands the kernels), as fp32 arrays."""
    w = class_set_weights(np.load(GOLDEN_CLASSES), tag) if tag == "K64_C5_nl" else load_weights(tag)
    return {k: round_bf16(w[k]) for k in KEYS if k in w and w[k] is not None}


def make_case(tag, N, seed=0):
    """x [N,K] (bf16-exact fp32), the rounded weights, and dense upstream gradients {pred [C], classes [N,C], A [N,C], B [C,K]}."""
    K, C, nonlinear = variant(tag)
    x = round_bf16(make_bag(4100 + 7 * N + K + seed, N, K))
    rng = np.random.default_rng(91 + N + K + seed)
    g = {"pred": rng.standard_normal(C).astype(np.float32), "classes": rng.standard_normal((N, C)).astype(np.float32),
         "A": rng.standard_normal((N, C)).astype(np.float32), "B": rng.standard_normal((C, K)).astype(np.float32)}
    return x, weights(tag), g


def query(x, p, nonlinear, dtype=np.float64, round_hidden=False):
    """H = relu(x W1^T + b1), Q = tanh(H W2^T + b2) (H = Q = the linear query when not nonlinear); round_hidden: H rounded
    once to bf16 in front of the second layer, as the bf16 forward does."""
    x = np.asarray(x, dtype)
    H = x @ np.asarray(p["q0_w"], dtype).T + np.asarray(p["q0_b"], dtype)
    if not nonlinear:
        return H, H
    H = np.maximum(H, 0)
    Hq = round_bf16(H).astype(dtype) if round_hidden else H
    return H, np.tanh(Hq @ np.asarray(p["q2_w"], dtype).T + np.asarray(p["q2_b"], dtype))


def forward(x, p, nonlinear, dtype=np.float64, round_hidden=False):
    """dsmil.py:46-62 (+ the fused FCLayer) for one bag, v = Identity: (classes, pred, A, B, idx)."""
    x = np.asarray(x, dtype)
    classes = x @ np.asarray(p["fc_w"], dtype).T + np.asarray(p["fc_b"], dtype)
    idx = classes.argmax(0)
    _, Q = query(x, p, nonlinear, dtype, round_hidden)
    s = Q @ Q[idx].T / np.sqrt(dtype(128.0))
    e = np.exp(s - s.max(0, keepdims=True))
    A = e / e.sum(0, keepdims=True)
    B = A.T @ x
    pred = np.einsum("ock,ck->o", np.asarray(p["fcc_w"], dtype), B) + np.asarray(p["fcc_b"], dtype)
    return classes, pred, A, B, idx


def formula(x, vals, p, A, B, idx, g, nonlinear, dtype=np.float64):
    """The header formulas of csrc/agg_bwd.hip with A [N,C], B [C,Kv], idx [C] as INPUTS.  g: upstream gradients "pred" [C]
    and optionally "classes" [N,C], "A" [N,C], "B" [C,Kv], "max" [C] (the sparse gradient of max_n classes[n,:])."""
    f = lambda t: np.asarray(t, dtype)
    x, A, B = f(x), f(A), f(B)
    V = x if vals is None else f(vals)
    idx = np.asarray(idx).reshape(-1)
    C = A.shape[1]
    g_pred = f(g["pred"]).reshape(-1)
    gB = np.einsum("o,ock->ck", g_pred, f(p["fcc_w"]))
    if g.get("B") is not None:
        gB = gB + f(g["B"])
    out = {"fcc_w": g_pred[:, None, None] * B[None], "fcc_b": g_pred.copy()}
    gA = V @ gB.T
    D = (gB * B).sum(1)
    if g.get("A") is not None:
        gA = gA + f(g["A"])
        D = D + (A * f(g["A"])).sum(0)
    gs = A * (gA - D) / np.sqrt(dtype(128.0))
    H, Q = query(x, p, nonlinear, dtype)
    gQ = gs @ Q[idx]
    for c in range(C):
        gQ[idx[c]] += gs[:, c] @ Q
    if nonlinear:
        gz2 = gQ * (1 - Q * Q)
        out["q2_w"], out["q2_b"] = gz2.T @ H, gz2.sum(0)
        gH = (gz2 @ f(p["q2_w"])) * (H > 0)
    else:
        gH = gQ
    out["q0_w"], out["q0_b"] = gH.T @ x, gH.sum(0)
    if g.get("classes") is not None or g.get("max") is not None:
        gw, gb = np.zeros((C, x.shape[1]), dtype), np.zeros(C, dtype)
        if g.get("classes") is not None:
            gw += f(g["classes"]).T @ x
            gb += f(g["classes"]).sum(0)
        if g.get("max") is not None:
            gm = f(g["max"]).reshape(-1)
            gw += gm[:, None] * x[idx]
            gb += gm
        out["fc_w"], out["fc_b"] = gw, gb
    out["vals"] = A @ gB
    return out


def formula_f64(x, vals, p, A, B, idx, g, nonlinear=True):
    return formula(x, vals, p, A, B, idx, g, nonlinear, np.float64)


def autograd_f64(x, p, g, nonlinear):
    """fp64 torch autograd of the reference expression (the arg-max indices are constants) with the dense upstream
    gradients g: the exact gradient at these rows and weights.  Returns (grads, (classes, pred, A, B, idx))."""
    xt = torch.from_numpy(np.asarray(x, np.float64))
    P = {k: torch.from_numpy(np.asarray(v, np.float64)).requires_grad_(True) for k, v in p.items()}
    c = xt @ P["fc_w"].T + P["fc_b"]
    idx = c.argmax(0)
    h = xt @ P["q0_w"].T + P["q0_b"]
    Q = torch.tanh(torch.relu(h) @ P["q2_w"].T + P["q2_b"]) if nonlinear else h
    A = torch.softmax(Q @ Q[idx].T / np.sqrt(128.0), 0)
    B = A.T @ xt
    pred = torch.einsum("ock,ck->o", P["fcc_w"], B) + P["fcc_b"]
    obj = (pred * torch.from_numpy(g["pred"]).double()).sum()
    for name, t in (("classes", c), ("A", A), ("B", B)):
        if g.get(name) is not None:
            obj = obj + (t * torch.from_numpy(g[name]).double()).sum()
    obj.backward()
    return ({k: v.grad.numpy() for k, v in P.items()},
            tuple(t.detach().numpy() for t in (c, pred, A, B, idx)))


def bar(ref):
    """The fp32 backward's own bar (tests/test_agg_bwd_gpu.py): 2e-4 of the tensor's max-abs + 2e-5."""
    return 2e-4 * float(np.abs(ref).max()) + 2e-5


def max_err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max())


@functools.lru_cache(maxsize=None)
def dev_host(tag, N):
    """Check (g): per parameter tensor, the deviation (as a share of the exact gradient's max-abs) between the exact
    gradient and the formula fed the A, B of a forward whose hidden layer is rounded to bf16 — what separates the bf16
    path's gradient from the fp32 path's on the same rows and weights, apart from accumulation order."""
    x, p, g = make_case(tag, N)
    _, _, nonlinear = variant(tag)
    exact, _ = autograd_f64(x, p, g, nonlinear)
    _, _, A, B, idx = forward(x, p, nonlinear, np.float64, round_hidden=True)
    got = formula_f64(x, None, p, A, B, idx, g, nonlinear)
    return {k: max_err(got[k], exact[k]) / max(float(np.abs(exact[k]).max()), 1e-300) for k in exact}
