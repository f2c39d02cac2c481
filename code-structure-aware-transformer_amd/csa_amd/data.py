"""Synthetic AST batches with the reference's relation encoding (no datasets offline).

The real pipeline parses code with tree-sitter and builds, per AST truncated to ``max_size``
nodes in pre-order (my_ast.py:129-143):

* L (ancestor/descendant relation): for every ancestor a and descendant c on a root-to-leaf
  path, L[a,c] = depth(c)-depth(a) and L[c,a] = -(depth(c)-depth(a)) (my_ast.py:223-263);
* T (sibling relation): for siblings i before j among one parent's children,
  T[i,j] = j_idx - i_idx and T[j,i] = -(j_idx - i_idx) (my_ast.py:232-270);
* zeros elsewhere (diagonal, unrelated pairs, padding);

and the collate step encodes them as ``mask = raw.eq(0)`` and ``idx = clamp(raw + 75, 0, 149)``
(dataset/base_data_set.py:33-36). This module generates random trees (uniform parent
attachment, at most 6 children per node) and produces exactly that encoding, vectorised
in numpy. The hot-path kernels consume the uint8 (B,N,N) relation/mask planes directly
(head stride 0), instead of the reference's repeated int64 (B,8,N,N) copies
(module/csa_trans.py:206-211).
"""
import numpy as np

PAD, UNK, BOS, EOS = 0, 1, 2, 3  # utils/vocab.py:10-13
REL_OFFSET, REL_MAX = 75, 149  # dataset/base_data_set.py:35-36


def random_tree(n, rng, max_children=6):
    """Random rooted tree with n nodes; returns parent[] in PRE-ORDER numbering (root = 0)."""
    parent = np.full(n, -1, dtype=np.int64)
    nchild = np.zeros(n, dtype=np.int64)
    children = [[] for _ in range(n)]
    for v in range(1, n):
        while True:
            p = int(rng.integers(0, v))
            if nchild[p] < max_children:
                break
        parent[v] = p
        nchild[p] += 1
        children[p].append(v)
    # pre-order renumbering (children in insertion order), as MyAst numbers nodes
    order = []
    stack = [0]
    while stack:
        v = stack.pop()
        order.append(v)
        stack.extend(reversed(children[v]))
    newid = np.empty(n, dtype=np.int64)
    newid[np.array(order)] = np.arange(n)
    par = np.full(n, -1, dtype=np.int64)
    for v in range(1, n):
        par[newid[v]] = newid[parent[v]]
    kids = [[] for _ in range(n)]
    for v in range(1, n):  # pre-order ids are increasing along sibling order
        kids[par[v]].append(v)
    return par, kids


def relation_matrices(par, kids, max_size):
    """Raw signed L/T matrices (max_size x max_size, float32) of one tree (my_ast.py:198-273)."""
    n = len(par)
    L = np.zeros((max_size, max_size), dtype=np.float32)
    T = np.zeros((max_size, max_size), dtype=np.float32)
    depth = np.zeros(n, dtype=np.int64)
    for v in range(1, n):
        depth[v] = depth[par[v]] + 1
    for c in range(1, n):
        a = par[c]
        while a >= 0:
            dist = depth[c] - depth[a]
            L[a, c] = dist
            L[c, a] = -dist
            a = par[a]
    for p in range(n):
        ch = kids[p]
        for i in range(len(ch)):
            for j in range(i + 1, len(ch)):
                T[ch[i], ch[j]] = j - i
                T[ch[j], ch[i]] = -(j - i)
    return L, T


def collate_relations(raw):
    """dataset/base_data_set.py:33-36 -> (idx uint8, mask bool)."""
    mask = raw == 0
    idx = np.clip(raw + REL_OFFSET, 0, REL_MAX).astype(np.uint8)
    return idx, mask


def relation_planes(parents, n_nodes, max_size, nthreads=None):
    """Native (csrc/csa_host.cpp: csa_ast_relations) relation planes of a batch of pre-order trees:
    parents (B, max_size) int32 (parent[v] < v, root -1), n_nodes (B,) -> L, T (B,N,N) uint8 relation
    indices and L_mask, T_mask (B,N,N) bool, identical to relation_matrices + collate_relations."""
    import ctypes
    import os
    from ._lib import check, lib
    parents = np.ascontiguousarray(parents, dtype=np.int32)
    n_nodes = np.ascontiguousarray(n_nodes, dtype=np.int32)
    B = parents.shape[0]
    out = [np.empty((B, max_size, max_size), np.uint8) for _ in range(4)]
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    nt = nthreads or min(16, os.cpu_count() or 1)
    check(lib().csa_ast_relations(p(parents), p(n_nodes), B, max_size, *(p(o) for o in out), nt),
          "csa_ast_relations")
    L, T, Lm, Tm = out
    return L, T, Lm.view(bool), Tm.view(bool)


TREE_WIDTH, TREE_HEIGHT = 8, 16  # dataset/fast_ast_data_set.py:136-137
TRIPLET_VOCAB = 1246  # module/csa_trans.py:141


def tree_levels(par):
    """(depth, sibling index) of every node of a pre-order parent array (parent[v] < v, root -1)."""
    n = len(par)
    depth = np.zeros(n, np.int64)
    child_idx = np.zeros(n, np.int64)
    nchild = np.zeros(n, np.int64)
    for v in range(1, n):
        p = par[v]
        depth[v] = depth[p] + 1
        child_idx[v] = nchild[p]
        nchild[p] += 1
    return depth, child_idx


def adjacency(par, max_size):
    """The reference's `adj` (dataset/fast_ast_data_set.py:127-128) of one tree: raw L in {-1, 0, 1} inside the
    n x n block, so True for parent / child pairs, on the diagonal and for every unrelated pair (raw L = 0), False for
    ancestors two or more levels apart; False outside the block. Symmetric and nearly dense."""
    n = len(par)
    adj = np.zeros((max_size, max_size), bool)
    adj[:n, :n] = True
    par = np.asarray(par, np.int64)
    idx = np.arange(n)
    anc = np.where(par >= 0, par[np.maximum(par, 0)], -1)  # the grandparent: distance 2
    while True:
        ok = anc >= 0
        if not ok.any():
            break
        adj[anc[ok], idx[ok]] = False
        adj[idx[ok], anc[ok]] = False
        anc = np.where(ok, par[np.maximum(anc, 0)], -1)
    return adj


def tree_positions(par, max_size):
    """The reference's tree_pos (dataset/fast_ast_data_set.py:84-104,136-147) of one tree, child_idx taken as the
    sibling index: a node's vector is one_hot(min(child_idx, 7), 8) followed by its parent's (the root's is empty),
    truncated to its last 128 entries and left-padded with zeros to 128. So the step into the node at depth d sets
    entry 128 - 8 d + child_idx, for d <= 16. (max_size, 128) fp32, zero rows beyond the tree."""
    n = len(par)
    depth, child_idx = tree_levels(par)
    W, D = TREE_WIDTH, TREE_WIDTH * TREE_HEIGHT
    tp = np.zeros((max_size, D), np.float32)
    for v in range(1, n):
        tp[v] = tp[par[v]]
        if depth[v] <= TREE_HEIGHT:
            tp[v, D - W * depth[v] + min(child_idx[v], W - 1)] = 1.0
    return tp


def triplet_ids(par, max_size):
    """Ids of the node triplets (level, parent's child_idx, child_idx) (dataset/fast_ast_data_set.py:47-50,116-122).
    The reference looks them up in node_triplet_dictionary_*.pt, which is not available offline; this is a SYNTHETIC
    vocabulary, the enumeration 2 + min(level, 15) * 64 + min(parent_idx, 7) * 8 + min(child_idx, 7) (< 1246), the
    root's id that of (0, 0, 0) and PAD beyond the tree. (max_size,) int64."""
    n = len(par)
    depth, child_idx = tree_levels(par)
    ids = np.full(max_size, PAD, np.int64)
    for v in range(n):
        pidx = child_idx[par[v]] if v > 0 else 0
        ids[v] = 2 + min(depth[v], 15) * 64 + min(pidx, 7) * 8 + min(child_idx[v], 7)
    return ids


def collect_fn(batch, nthreads=None):
    """BaseASTDataSet.collect_fn (dataset/base_data_set.py:20-75) for the accelerated path: `batch` is a
    list of (item, _) with item dicts holding the preprocessed per-AST tensors -- src_seq, tgt_seq,
    target (equal lengths across the batch), raw fp32 L / T (N, N) from split_matrices.npz, num_node.
    Returns (namespace, target) like the reference's (Data, target), with the relation planes encoded
    by the native csa_collate_relations as the uint8 L, T and bool L_mask, T_mask the kernels read
    (idx = clamp(raw + 75, 0, 149), mask = raw == 0). The ablation fields of the reference (adj (N, N) bool,
    tree_pos (n, 128) zero-padded to N rows as the reference pads to 150, triplet (N,)) are collated when every
    item has all three."""
    import ctypes
    import os
    from types import SimpleNamespace

    import torch
    from ._lib import check, lib
    items = [it for it, _ in batch]
    stack = lambda k: torch.stack([torch.as_tensor(it[k]) for it in items], 0)
    Lr = stack("L").to(torch.float32).contiguous()
    Tr = stack("T").to(torch.float32).contiguous()
    if Lr.shape != Tr.shape:
        raise ValueError("L and T must have the same shape")
    outs = [torch.empty(Lr.shape, dtype=torch.uint8) for _ in range(4)]
    nt = nthreads or min(16, os.cpu_count() or 1)
    check(lib().csa_collate_relations(ctypes.c_void_p(Lr.data_ptr()), ctypes.c_void_p(Tr.data_ptr()), Lr.numel(),
                                      *(ctypes.c_void_p(o.data_ptr()) for o in outs), nt), "csa_collate_relations")
    L, T, Lm, Tm = outs
    target = stack("target")
    data = SimpleNamespace(src_seq=stack("src_seq"), tgt_seq=stack("tgt_seq"), target=target, L=L, T=T,
                           L_mask=Lm.view(torch.bool), T_mask=Tm.view(torch.bool),
                           num_node=torch.tensor([int(it["num_node"]) for it in items]))
    if all(k in it for it in items for k in ("adj", "tree_pos", "triplet")):
        N = Lr.shape[1]
        data.adj = stack("adj").to(torch.bool)
        tps = [torch.as_tensor(it["tree_pos"], dtype=torch.float32) for it in items]
        data.tree_pos = torch.stack([torch.cat([t, t.new_zeros(N - t.shape[0], t.shape[1])], 0) for t in tps], 0)
        data.triplet = stack("triplet").to(torch.int64)
    return data, target


def collate_parents(batch):
    """collect_fn's counterpart for items that store a parent array instead of the raw L / T matrices: `batch` is a
    list of (item, _) with item dicts holding src_seq, tgt_seq, target (equal lengths across the batch), num_node and
    parents, the (n,) or (N,) parent array of the AST (parent[0] = -1, 0 <= parent[v] < v). Returns (namespace, target)
    with parents (B, N) int32 (N = src_seq's length, -1 beyond an item's array) and num_node (B,) int32 in place of
    every structural field: 4 N bytes per AST instead of 4 N^2. CSATrans.process_data builds what its use_pegen reads
    from them on the batch's device (batch_ops.ast_batch)."""
    from types import SimpleNamespace

    import torch
    items = [it for it, _ in batch]
    stack = lambda k: torch.stack([torch.as_tensor(it[k]) for it in items], 0)
    src = stack("src_seq")
    N = src.shape[1]
    parents = torch.full((len(items), N), -1, dtype=torch.int32)
    for b, it in enumerate(items):
        p = torch.as_tensor(it["parents"]).to(torch.int32).reshape(-1)[:N]
        parents[b, :p.numel()] = p
    target = stack("target")
    data = SimpleNamespace(src_seq=src, tgt_seq=stack("tgt_seq"), target=target, parents=parents,
                           num_node=torch.tensor([int(it["num_node"]) for it in items], dtype=torch.int32))
    return data, target


def synthetic_batch(batch, max_size=150, seed=1, min_nodes=None, max_nodes=None, src_vocab=10000,
                    tgt_vocab=20000, max_tgt_len=50, native=True, ablation_fields=False, planes=True):
    """A batch of synthetic ASTs. Returns a dict of numpy arrays:

    L, T (B,N,N) uint8 relation indices; L_mask, T_mask (B,N,N) bool; src_mask (B,N) bool
    (True = padded node); num_node (B,); src_seq (B,N) int64 in [2, src_vocab) with PAD beyond
    num_node; tgt_seq/target (B, max_tgt_len-1) int64 (BOS ... EOS, PAD). Relation planes come from
    the native builder (relation_planes) unless native=False. ablation_fields=True adds what the structure-encoding
    ablations read, built from the same trees: adj (B,N,N) bool (adjacency), tree_pos (B,N,128) fp32
    (tree_positions) and triplet (B,N) int64 (triplet_ids, a synthetic vocabulary). planes=False returns, from the same
    RNG draws, parents (B,N) int32 (-1 beyond num_node) in place of every structural field (L, T, the masks and the
    ablation fields): the batch that batch_ops.ast_batch completes on the device."""
    rng = np.random.default_rng(seed)
    lo = max_size if min_nodes is None else min_nodes
    hi = max_size if max_nodes is None else max_nodes
    L = np.zeros((batch, max_size, max_size), np.uint8)
    T = np.zeros_like(L)
    Lm = np.zeros((batch, max_size, max_size), bool)
    Tm = np.zeros_like(Lm)
    nn = np.zeros(batch, np.int64)
    src = np.zeros((batch, max_size), np.int64)
    tgt = np.zeros((batch, max_tgt_len), np.int64)
    parents = np.full((batch, max_size), -1, np.int32)
    for b in range(batch):
        n = int(rng.integers(lo, hi + 1))
        par, _ = random_tree(n, rng)
        parents[b, :n] = par
        nn[b] = n
        src[b, :n] = rng.integers(2, src_vocab, n)
        tl = int(rng.integers(5, max_tgt_len - 1))
        tgt[b, 0] = BOS
        tgt[b, 1:tl + 1] = rng.integers(4, tgt_vocab, tl)
        tgt[b, tl + 1] = EOS
    src_mask = np.arange(max_size)[None, :] >= nn[:, None]
    if not planes:
        return dict(parents=parents, num_node=nn, src_seq=src, src_mask=src_mask, tgt_seq=tgt[:, :-1], target=tgt[:, 1:])
    if native:
        L, T, Lm, Tm = relation_planes(parents, nn, max_size)
    else:  # the Python restatement (tests compare the two)
        for b in range(batch):
            n = int(nn[b])
            kids = [[] for _ in range(n)]
            for v in range(1, n):
                kids[parents[b, v]].append(v)
            rl, rt = relation_matrices(parents[b, :n].astype(np.int64), kids, max_size)
            L[b], Lm[b] = collate_relations(rl)
            T[b], Tm[b] = collate_relations(rt)
    out = dict(L=L, T=T, L_mask=Lm, T_mask=Tm, num_node=nn, src_seq=src, src_mask=src_mask,
               tgt_seq=tgt[:, :-1], target=tgt[:, 1:])
    if ablation_fields:
        pars = [parents[b, :int(nn[b])].astype(np.int64) for b in range(batch)]
        out["adj"] = np.stack([adjacency(p, max_size) for p in pars])
        out["tree_pos"] = np.stack([tree_positions(p, max_size) for p in pars])
        out["triplet"] = np.stack([triplet_ids(p, max_size) for p in pars])
    return out
