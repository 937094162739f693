"""float64 torch restatement of the cross-view heat-map fusion (csrc/view_fusion.hip), written from its two formulas:

    F[b,i,k,:] = w_self * H[b,i,k,:] + w_other * sum over j != i of  H[b,j,k,:] @ W[n(i,j)]^T
    n(i,j) = i*(V-1) + (rank of j among the views other than i, ascending)

Gradients come from autograd on this function. `bounds` are the forward-error bounds the GPU tests hold the kernels to."""
import numpy as np
import torch

EPS = 2.0 ** -24          # unit round-off of float32


def pair_index(i, j, V):
    others = [v for v in range(V) if v != i]
    return i * (V - 1) + others.index(j)


def fusion_ref(H, Ws, w_self=0.4, w_other=0.2):
    """H (B, V, K, P) float64, Ws: V * (V - 1) tensors (P, P) float64 -> F (B, V, K, P)"""
    B, V, K, P = H.shape
    out = []
    for i in range(V):
        acc = w_self * H[:, i]
        for j in range(V):
            if j != i:
                acc = acc + w_other * (H[:, j] @ Ws[pair_index(i, j, V)].t())
        out.append(acc)
    return torch.stack(out, 1)


def fusion_loops(H, Ws, w_self=0.4, w_other=0.2):
    """the same with explicit Python loops over every index (numpy float64): the check of fusion_ref itself"""
    H = np.asarray(H, dtype=np.float64)
    B, V, K, P = H.shape
    F = np.zeros_like(H)
    for b in range(B):
        for i in range(V):
            others = [v for v in range(V) if v != i]
            for k in range(K):
                for o in range(P):
                    s = w_self * H[b, i, k, o]
                    for rank, j in enumerate(others):
                        W = np.asarray(Ws[i * (V - 1) + rank], dtype=np.float64)
                        for p in range(P):
                            s += w_other * H[b, j, k, p] * W[o, p]
                    F[b, i, k, o] = s
    return F


def inputs(B, V, K, P, seed):
    """seeded inputs of the GPU tests: positive H rows (a softmax), W uniform in +-1/sqrt(P), a gradient dF of N(0, 1);
    float32 values as float64 tensors"""
    rng = np.random.default_rng(seed)
    z = rng.normal(0.0, 1.0, (B, V, K, P))
    e = np.exp(z - z.max(-1, keepdims=True))
    H = (e / e.sum(-1, keepdims=True)).astype(np.float32).astype(np.float64)
    Ws = [(rng.uniform(-1.0, 1.0, (P, P)) / np.sqrt(P)).astype(np.float32).astype(np.float64)
          for _ in range(V * (V - 1))]
    dF = rng.normal(0.0, 1.0, (B, V, K, P)).astype(np.float32).astype(np.float64)
    return torch.from_numpy(H), [torch.from_numpy(w) for w in Ws], torch.from_numpy(dF)


def forward_bound(H, Ws, w_self=0.4, w_other=0.2):
    """elementwise bound on |F_f32 - F_exact|: an f32 dot product of n terms differs from the exact one by at most
    about n * 2^-24 * sum|a||b|; n = (V - 1) * P, and the factor 2 covers the output rounding and the summation order"""
    B, V, K, P = H.shape
    mag = fusion_ref(H.abs(), [w.abs() for w in Ws], w_self, w_other)
    return 2.0 * (V - 1) * P * EPS * mag


def dh_bound(dF, Ws, w_self=0.4, w_other=0.2):
    """the same for dH = w_self dF_j + w_other sum_{i != j} dF_i @ W[n(i,j)]: reduction length (V - 1) * P"""
    B, V, K, P = dF.shape
    a = dF.abs()
    out = []
    for j in range(V):
        acc = w_self * a[:, j]
        for i in range(V):
            if i != j:
                acc = acc + w_other * (a[:, i] @ Ws[pair_index(i, j, V)].abs())
        out.append(acc)
    return 2.0 * (V - 1) * P * EPS * torch.stack(out, 1)


def dw_bounds(H, dF, w_other=0.2):
    """for dW[n(i,j)] = w_other * dF[:,i]^T @ H[:,j]: reduction length B * K"""
    B, V, K, P = H.shape
    out = {}
    for i in range(V):
        for j in range(V):
            if j != i:
                a = dF[:, i].abs().reshape(B * K, P)
                h = H[:, j].abs().reshape(B * K, P)
                out[pair_index(i, j, V)] = 2.0 * (B * K) * EPS * w_other * (a.t() @ h)
    return out
