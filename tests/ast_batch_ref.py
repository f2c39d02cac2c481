"""Trees and expected values for the batch-preparation tests (csa_amd.batch_ops.ast_batch): every expectation comes
from the host builders (data.relation_planes, adjacency, tree_positions, triplet_ids), the Python restatement
(data.relation_matrices) or the committed goldens, never from the kernel."""
import functools

import numpy as np

ALL = ("L", "T", "L_mask", "T_mask", "adj", "tree_pos", "triplet")


def chain(n):
    """0 <- 1 <- 2 ...: depths 0 .. n - 1."""
    return np.arange(-1, n - 1, dtype=np.int32)


def star(n):
    """n - 1 children of the root: child indices 0 .. n - 2."""
    p = np.zeros(n, np.int32)
    p[0] = -1
    return p


def bfs_tree(n, seed, max_children=4):
    """A random tree numbered level by level (parent[v] < v holds, pre-order does not: a node's subtree is not a run
    of consecutive ids). Returns (parents int32, kids)."""
    rng = np.random.default_rng(seed)
    par = np.full(n, -1, np.int32)
    kids = [[] for _ in range(n)]
    nxt, v = 1, 0
    while nxt < n:  # node v, in id order, takes the next 1..max_children ids as its children
        k = int(rng.integers(1, max_children + 1)) if v > 0 else max_children
        for _ in range(min(k, n - nxt)):
            par[nxt] = v
            kids[v].append(nxt)
            nxt += 1
        v += 1
    return par, kids


def pad(trees, N):
    """A list of parent arrays -> (parents (B, N) int32 with -1 beyond each tree, num_node (B,) int32)."""
    parents = np.full((len(trees), N), -1, np.int32)
    for b, p in enumerate(trees):
        parents[b, :len(p)] = p
    return parents, np.array([len(p) for p in trees], np.int32)


def host_fields(parents, num_node):
    """Every field from the host builders, as numpy arrays (masks and adj bool)."""
    from csa_amd import data as D
    B, N = parents.shape
    n = np.clip(np.asarray(num_node, np.int64), 0, N)
    L, T, Lm, Tm = D.relation_planes(parents, n, N)
    pars = [parents[b, :n[b]].astype(np.int64) for b in range(B)]
    return dict(L=L, T=T, L_mask=Lm, T_mask=Tm, adj=np.stack([D.adjacency(p, N) for p in pars]),
                tree_pos=np.stack([D.tree_positions(p, N) for p in pars]),
                triplet=np.stack([D.triplet_ids(p, N) for p in pars]))


def empty_fields(N):
    """What a malformed tree gets: the empty tree's fields."""
    return dict(L=np.full((N, N), 75, np.uint8), T=np.full((N, N), 75, np.uint8), L_mask=np.ones((N, N), bool),
                T_mask=np.ones((N, N), bool), adj=np.zeros((N, N), bool), tree_pos=np.zeros((N, 128), np.float32),
                triplet=np.zeros(N, np.int64))


@functools.lru_cache(maxsize=None)
def shapes_case(N):
    """B = 3 trees in N slots: a full random tree, a short chain-and-star mix, a BFS-numbered tree; with their host
    fields (computed once, treated as read-only)."""
    from csa_amd.data import random_tree
    rng = np.random.default_rng(1000 + N)
    full, _ = random_tree(N, rng)
    m = max(1, N - 1)  # one slot short of full: a padded row and column
    half = max(1, m // 2)
    mix = np.concatenate([chain(half), np.zeros(m - half, np.int32)])  # a chain, then children of the root
    third, _ = bfs_tree(max(1, (2 * N) // 3), 7 + N)
    parents, nn = pad([full.astype(np.int32), mix.astype(np.int32), third], N)
    return parents, nn, host_fields(parents, nn)


def assert_fields_equal(got, want, b=None, fields=ALL):
    """Bitwise comparison of a namespace of tensors (or dict of arrays) against expected numpy arrays."""
    for f in fields:
        g = getattr(got, f) if not isinstance(got, dict) else got[f]
        g = g.cpu().numpy() if hasattr(g, "cpu") else np.asarray(g)
        w = want[f]
        if b is not None:
            g = g[b]
        assert g.dtype == w.dtype, (f, g.dtype, w.dtype)
        np.testing.assert_array_equal(g, w, err_msg=f)
