"""Shared inputs and fp64 references of the structure-encoding tests (test_pe_modes_cpu.py, test_pe_modes_gpu.py):
the Laplacian eigenvector batch with its invariants, and the tree positional encoding in fp64 autograd."""
import functools

import numpy as np
import torch

U = 2.0 ** -24          # fp32 unit roundoff
GAP = 1e-2              # eigenvalues closer than this belong to one cluster
LAP_N = 150
LAP_SIZES = (1, 2, 3, 12, 37, 64, 65, 150)  # n = 1, the bye of odd n, the wave-size boundary, the largest size
LAP_SEED = 5


@functools.lru_cache(maxsize=None)
def lap_batch(N=LAP_N, sizes=LAP_SIZES, seed=LAP_SEED):
    """adj (B, N, N) bool with the reference's adjacency of one random tree of each size in its n x n block and
    garbage ones outside it, and num_node (B,) int64. Cached: do not modify."""
    from csa_amd.data import adjacency, random_tree
    rng = np.random.default_rng(seed)
    adj = rng.random((len(sizes), N, N)) < 0.5  # garbage outside the blocks
    for b, n in enumerate(sizes):
        par, _ = random_tree(n, rng)
        adj[b, :n, :n] = adjacency(par, N)[:n, :n]
    adj.setflags(write=False)
    return adj, np.array(sizes, np.int64)


def laplacian64(adj_b, n):
    """The reference's formula (module/base_seq2seq.py:22-33) in fp64: L = I - D^-1/2 A D^-1/2."""
    A = np.asarray(adj_b[:n, :n] != 0, np.float64)
    dinv = np.clip(A.sum(1), 1, None) ** -0.5
    return np.eye(n) - dinv[:, None] * A * dinv[None, :]


@functools.lru_cache(maxsize=None)
def lap_reference(N=LAP_N, sizes=LAP_SIZES, seed=LAP_SEED):
    """Per AST (L, eigenvalues, eigenvectors) in fp64 (numpy eigh). Cached: do not modify."""
    adj, nn_ = lap_batch(N, sizes, seed)
    out = []
    for b, n in enumerate(nn_):
        L = laplacian64(adj[b], int(n))
        w, U_ = np.linalg.eigh(L)
        out.append((L, w, U_))
    return out


def clusters(w, gap=GAP):
    """Index ranges [lo, hi) of the ascending eigenvalues w split wherever two neighbours are >= gap apart."""
    cuts = [0] + [i + 1 for i in range(len(w) - 1) if w[i + 1] - w[i] >= gap] + [len(w)]
    return [(cuts[i], cuts[i + 1]) for i in range(len(cuts) - 1)]


def lap_quantities(L, w, U_, V, lam):
    """The four measured quantities of one AST: residual max|L V - V diag(lam)|, orthogonality max|V^T V - I|,
    eigenvalue error max|lam - w| and the worst projector error max|V_c V_c^T - U_c U_c^T| over the clusters of w."""
    V = np.asarray(V, np.float64)
    lam = np.asarray(lam, np.float64)
    n = len(w)
    res = np.abs(L @ V - V * lam[None, :]).max()
    orth = np.abs(V.T @ V - np.eye(n)).max()
    eig = np.abs(lam - w).max()
    proj = max(np.abs(V[:, lo:hi] @ V[:, lo:hi].T - U_[:, lo:hi] @ U_[:, lo:hi].T).max() for lo, hi in clusters(w))
    return res, orth, eig, proj


def lap_bounds(n):
    """The bounds of those four quantities for a backward-stable fp32 solver of M = L + I, |M|_2 < 3: four times
    n u |M| for the residual and the eigenvalues, 4 n u for the orthogonality, Davis-Kahan over the gap for the
    projectors."""
    return 12 * n * U, 4 * n * U, 12 * n * U, 2 * (12 * n * U) / GAP


def check_sign_rule(V):
    """Every column's largest-magnitude entry (the first on ties) is positive."""
    V = np.asarray(V)
    idx = np.abs(V).argmax(0)
    assert (V[idx, np.arange(V.shape[1])] > 0).all()


def check_lap_result(pe, ev, adj, nn_, ref, report=None):
    """Everything asserted of a lap_pe result (numpy arrays) against the fp64 reference `ref` of the same batch."""
    B, N, P = pe.shape
    for b in range(B):
        n = int(nn_[b])
        L, w, U_ = ref[b]
        V, lam = pe[b, :n, :n], ev[b, :n]
        q = lap_quantities(L, w, U_, V, lam)
        bd = lap_bounds(n)
        if report is not None:
            report.append((n,) + tuple(q) + tuple(bd))
        print(f"n={n}: residual {q[0]:.2e} (<= {bd[0]:.2e}), orthogonality {q[1]:.2e} (<= {bd[1]:.2e}), "
              f"eigenvalues {q[2]:.2e} (<= {bd[2]:.2e}), projectors {q[3]:.2e} (<= {bd[3]:.2e})")
        for name, x, y in zip(("residual", "orthogonality", "eigenvalue", "projector"), q, bd):
            assert x <= y, (n, name, x, y)
        assert (np.diff(lam) >= 0).all(), n
        check_sign_rule(V)
        mask = np.ones((N, P), bool)
        mask[:n, :n] = False
        assert (pe[b][mask] == 0).all() and (ev[b, n:] == 0).all(), n


# ---- tree positional encoding ----

def tree_pos_case(rows_shape, F, seed, binary=True, zero_p=False):
    """pos (*rows_shape, 128), p (F,) with values in (0.7, 0.999) (optionally an exact 0.0 first) and the upstream
    gradient g, all fp32 CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    pos = (torch.rand(*rows_shape, 128, generator=g) < 0.15).float()
    if not binary:
        pos = pos * torch.randn(*rows_shape, 128, generator=g)
    p = 0.7 + 0.299 * torch.rand(F, generator=g)
    if zero_p:
        p[0] = 0.0
    dout = torch.randn(*rows_shape, 128 * F, generator=g)
    return pos, p, dout


def tree_pos_reference64(pos, p, dout, depth=16, width=8):
    """fp64 autograd of the reference's expressions: (out, dp, bound), bound[f] = R u sum|terms| with the terms
    pos[r, j] dout[r, j F + f] dw[j, f]/dp_f of dp_f's sum and R the row count: the worst-case error of an fp32 sum
    of R terms."""
    from csa_amd.pe_ops import tree_pos_reference, tree_weights
    F = p.numel()
    d_model = depth * width * F
    p64 = p.double().requires_grad_(True)
    out = tree_pos_reference(pos.double(), p64, depth, width, d_model)
    (dp,) = torch.autograd.grad(out, p64, dout.double())
    # dw[j, f] / dp_f, column by column
    q = p.double().requires_grad_(True)
    w = tree_weights(q, depth, width, d_model)  # (C, F)
    dw = torch.stack([torch.autograd.grad(w[j].sum(), q, retain_graph=True)[0] for j in range(depth * width)])  # (C, F)
    R = pos.reshape(-1, depth * width).shape[0]
    S = (pos.double().reshape(R, -1, 1) * dout.double().reshape(R, depth * width, F)).abs().sum(0)  # (C, F)
    bound = R * U * (S * dw.abs()).sum(0)
    return out.detach(), dp.detach(), bound
