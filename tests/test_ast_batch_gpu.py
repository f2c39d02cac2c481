"""batch_ops.ast_batch on the GPU (csrc/csa_batch.hip): every field bitwise against the host builders and the
committed goldens, at every size and alignment class of the store path, with malformed trees, and through the model."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ast_batch_ref as R
from conftest import has_gpu
from golden_inputs import fill_params_deterministic

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs GPU")]


def _device(parents, nn, fields=R.ALL, **kw):
    from csa_amd.batch_ops import ast_batch
    return ast_batch(torch.from_numpy(np.ascontiguousarray(parents)).cuda(), torch.from_numpy(np.asarray(nn)).cuda(),
                     fields=fields, backend="device", **kw)


def test_golden_trees(golden):
    """The 12 trees of tests/golden/ast_relations.npz at N = 150 (sizes 1, 2, 3, 17, 60, 90, 149, 150; longer trees
    truncated to 150): the planes against the reference's own outputs, the other fields against the host builders."""
    z = golden("ast_relations")
    r = _device(z["parents"], z["n_nodes"], check=True)
    R.assert_fields_equal(r, z, fields=("L", "T", "L_mask", "T_mask"))
    R.assert_fields_equal(r, R.host_fields(z["parents"], z["n_nodes"]))
    assert r.status.tolist() == [0] * 12 and r.num_node.tolist() == z["n_nodes"].tolist()
    assert r.rel.shape == (12, 2, 150, 150) and r.L.data_ptr() == r.rel.data_ptr()
    assert r.T_mask.data_ptr() == r.rel_mask[:, 1].data_ptr() and r.L_mask.dtype == torch.bool


def test_golden_tree_pos_rows(golden):
    """tests/golden/tree_pos_ref.npz, the reference's gen_tree_positions rows (a tree deeper than 16 among them)."""
    z = golden("tree_pos_ref")
    trees = [z[f"par{i}"].astype(np.int32) for i in range(len([k for k in z if k.startswith("par")]))]
    parents, nn = R.pad(trees, 150)
    tp = _device(parents, nn, fields=("tree_pos",)).tree_pos.cpu().numpy()
    for i, p in enumerate(trees):
        np.testing.assert_array_equal(tp[i, :len(p)], z[f"tree_pos{i}"])
        assert not tp[i, len(p):].any()


def test_chain_star_empty_and_overlong():
    """A 150-node chain (depths to 149: both clamp ends of L, tree_pos past depth 16, triplet's level cap), a star
    that fills the 150 slots (149 children: T saturates at both ends, child indices past 7), n = 0, and num_node > N."""
    from csa_amd.data import random_tree
    N = 150
    rnd, _ = random_tree(N, np.random.default_rng(3))
    parents, nn = R.pad([R.chain(N), R.star(N), R.chain(N), rnd.astype(np.int32)], N)
    nn = np.array([N, N, 0, 100000], np.int32)  # AST 2 is empty (its parent array is ignored), AST 3 claims too many
    want = R.host_fields(parents, nn)
    assert want["L"][0].min() == 0 and want["L"][0].max() == 149 and want["T"][1].min() == 0 and want["T"][1].max() == 149
    assert want["tree_pos"][0, 149].sum() == 16 and want["triplet"][1].max() == 2 + 64 + 7
    r = _device(parents, nn, check=True)
    R.assert_fields_equal(r, want)
    R.assert_fields_equal(r, R.empty_fields(N), b=2)
    assert r.num_node.tolist() == [N, N, 0, N]


@pytest.mark.parametrize("N", [1, 2, 37, 150])
def test_sizes_and_unaligned_planes(N):
    """B = 3 in (B, 2, N, N) buffers: N = 37 makes every plane of 1369 bytes start at another alignment mod 4,
    N = 150 gives 150-byte rows and two workgroups per AST, N = 1 and 2 planes shorter than a dword. A full tree, a
    chain-and-star mix one node short of N and a BFS-numbered tree, every field."""
    parents, nn, want = R.shapes_case(N)
    r = _device(parents, nn, check=True)
    if N == 37:
        assert {t.data_ptr() % 4 for t in (r.rel[0, 0], r.rel[0, 1], r.rel[1, 0], r.rel[1, 1])} == {0, 1, 2, 3}
    R.assert_fields_equal(r, want)


def test_long_asts():
    """N = 1024 (the long-AST config; 64 workgroups per AST): a random tree and a chain."""
    from csa_amd.data import random_tree
    N = 1024
    rnd, _ = random_tree(N, np.random.default_rng(9))
    parents, nn = R.pad([rnd.astype(np.int32), R.chain(N)], N)
    want = R.host_fields(parents, nn)
    r = _device(parents, nn, check=True)
    R.assert_fields_equal(r, want)


def test_bfs_numbered_tree_against_the_python_restatement():
    """Topological, not pre-order, ids: ancestors cannot be read off the ids."""
    from csa_amd.data import collate_relations, relation_matrices
    par, kids = R.bfs_tree(150, 5)
    rl, rt = relation_matrices(par.astype(np.int64), kids, 150)
    (L, Lm), (T, Tm) = collate_relations(rl), collate_relations(rt)
    parents, nn = R.pad([par], 150)
    r = _device(parents, nn, check=True)
    R.assert_fields_equal(r, dict(L=L, T=T, L_mask=Lm, T_mask=Tm), b=0, fields=("L", "T", "L_mask", "T_mask"))
    R.assert_fields_equal(r, R.host_fields(parents, nn))


@pytest.mark.parametrize("field", R.ALL)
def test_each_field_alone_leaves_the_others_untouched(field):
    """The C entry point with one output pointer set: that buffer is exact, and sentinel-filled buffers of every
    other field, which the call is not given, keep their sentinels (as does the slack around the requested one)."""
    from csa_amd import _lib
    parents, nn, want = R.shapes_case(37)
    B, N = parents.shape
    dev = torch.device("cuda")
    dtypes = dict(L=torch.uint8, T=torch.uint8, L_mask=torch.uint8, T_mask=torch.uint8, adj=torch.uint8,
                  tree_pos=torch.float32, triplet=torch.int64)
    shapes = dict(tree_pos=(B, N, 128), triplet=(B, N))
    GUARD = 16  # elements of slack on both sides of every buffer
    flat = {f: torch.full((int(np.prod(shapes.get(f, (B, N, N)))) + 2 * GUARD,), 0x5A, dtype=dtypes[f], device=dev)
            for f in R.ALL}
    body = {f: flat[f][GUARD:-GUARD].view(shapes.get(f, (B, N, N))) for f in R.ALL}
    par, n32 = torch.from_numpy(parents).cuda(), torch.from_numpy(nn).cuda()
    status = torch.full((B,), 7, dtype=torch.int32, device=dev)
    args = _lib.AstBatchArgs(B=B, N=N, parents=par.data_ptr(), num_node=n32.data_ptr(), status=status.data_ptr())
    setattr(args, field, body[field].data_ptr())
    _lib.check(_lib.lib().csa_ast_batch(ctypes.byref(args), None), "csa_ast_batch")
    torch.cuda.synchronize()
    assert status.tolist() == [0] * B
    got = body[field].cpu().numpy()
    np.testing.assert_array_equal(got.view(want[field].dtype) if got.dtype == np.uint8 else got, want[field])
    for f in R.ALL:
        if f != field:
            assert bool((flat[f] == 0x5A).all()), f
    assert bool((flat[field][:GUARD] == 0x5A).all()) and bool((flat[field][-GUARD:] == 0x5A).all())


def test_malformed_tree_is_contained():
    """Bad ids that stay below N (parent[2] = 2, parent[3] = 5: in bounds as indices, wrong as a tree): status 1 for
    that AST alone, the empty tree's fields for it, exact neighbours; and check=True raises."""
    from csa_amd._lib import CsaError
    parents, nn, want = R.shapes_case(37)
    parents = parents.copy()
    parents[1, 2], parents[1, 3] = 2, 5
    r = _device(parents, nn)
    assert r.status.tolist() == [0, 1, 0]
    R.assert_fields_equal(r, R.empty_fields(37), b=1)
    for b in (0, 2):
        R.assert_fields_equal(r, {k: v[b] for k, v in want.items()}, b=b)
    with pytest.raises(CsaError, match="pre-order"):
        _device(parents, nn, check=True)
    # ids far outside the array, a negative non-root parent and a root with a parent are refused the same way
    for v, p in ((5, 2 ** 31 - 1), (5, -3), (0, 0), (4, 4)):
        q = R.shapes_case(37)[0].copy()
        q[2, v] = p
        r = _device(q, nn, fields=("L", "triplet"))
        assert r.status.tolist() == [0, 0, 1], (v, p)
        R.assert_fields_equal(r, R.empty_fields(37), b=2, fields=("L", "triplet"))
        R.assert_fields_equal(r, {k: w[0] for k, w in want.items()}, b=0, fields=("L", "triplet"))


def test_auto_backend_and_host_agree_on_device_tensors():
    """backend="auto" on CUDA tensors is the kernel; backend="host" returns the same fields on the device."""
    from csa_amd.batch_ops import ast_batch
    parents, nn, want = R.shapes_case(37)
    p, n = torch.from_numpy(parents).cuda(), torch.from_numpy(nn).cuda()
    a = ast_batch(p.to(torch.int64), n.to(torch.int64), fields=R.ALL)  # int64 inputs are converted
    h = ast_batch(p, n, fields=R.ALL, backend="host")
    for f in R.ALL:
        assert getattr(h, f).is_cuda and torch.equal(getattr(a, f), getattr(h, f)), f
    R.assert_fields_equal(a, want)


TINY = dict(src_vocab_size=50, tgt_vocab_size=60, hidden_size=64, num_heads=8, num_layers=1, sbm_layers=2,
            dim_feed_forward=128, dropout=0.2, pe_dim=32, pegen_dim=128, sbm_enc_dim=512, clusters=[10, 12],
            full_att=False)
OVERRIDES = {"pegen": {}, "laplacian": {}, "sequential": dict(pe_dim=0), "treepos": dict(pegen_dim=256), "triplet": {}}


@pytest.mark.parametrize("mode", list(OVERRIDES))
def test_model_forward_from_parents_equals_host_built_batch(mode):
    """The tiny CSATrans in eval mode: the forward from a parents-only batch equals the forward from the host-built
    batch bitwise (same weights, same uniforms); for pegen the data.rel path also equals the stacked path on the
    device-built planes."""
    from csa_amd.batch_ops import ast_batch
    from csa_amd.data import synthetic_batch
    from csa_amd.model import CSATrans, batch_to_device
    kw = dict(batch=3, max_size=37, seed=21, min_nodes=5, max_nodes=37, src_vocab=50, tgt_vocab=60, max_tgt_len=9)
    dev = torch.device("cuda")
    m = CSATrans(**{**TINY, **OVERRIDES[mode]}, use_pegen=mode)
    fill_params_deterministic(m, 90)
    m = m.to(dev).eval()
    g = torch.Generator().manual_seed(5)
    us = [torch.rand(3, 8, 37, 37, generator=g).to(dev) for _ in range(2)]

    def run(x):
        for i in range(2):
            getattr(m.SBM, f"transformer_{i}").mha.attn.uniforms = us[i]
        with torch.no_grad():
            out, sparsity, pe, _, _ = m(x)
        return out, sparsity, pe

    full, _ = batch_to_device(synthetic_batch(ablation_fields=True, **kw), dev)
    slim, _ = batch_to_device(synthetic_batch(planes=False, **kw), dev)
    assert not hasattr(slim, "L") and not hasattr(full, "parents")
    ref, got = run(full), run(slim)
    assert bool(torch.isfinite(ref[0]).all())
    for a, b in zip(ref, got):
        if a is not None:
            assert torch.equal(torch.as_tensor(a), torch.as_tensor(b))
    if mode == "pegen":
        assert hasattr(slim, "rel") and hasattr(slim, "rel_mask") and not hasattr(slim, "adj")
        built = ast_batch(slim.parents, slim.num_node)
        stacked = SimpleNamespace(src_seq=slim.src_seq, tgt_seq=slim.tgt_seq, L=built.L, T=built.T, L_mask=built.L_mask,
                                  T_mask=built.T_mask)  # no data.rel: CSE.forward stacks, as for a host-built batch
        for a, b in zip(ref, run(stacked)):
            assert torch.equal(torch.as_tensor(a), torch.as_tensor(b))
