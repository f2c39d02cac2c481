"""batch_ops.ast_batch without a GPU: the host backend against the reference's pinned outputs and the Python
restatement, its validation, and the parents-only batches of data.py. Every comparison is bitwise."""
import numpy as np
import pytest
import torch

import ast_batch_ref as R


def _host(parents, nn, fields=R.ALL, **kw):
    from csa_amd.batch_ops import ast_batch
    return ast_batch(torch.from_numpy(np.ascontiguousarray(parents)), torch.from_numpy(np.asarray(nn)), fields=fields,
                     **kw)


def test_host_backend_equals_golden_planes(golden):
    """tests/golden/ast_relations.npz: MyAst.__get_matrices + collect_fn on 12 trees (sizes 1 .. 150, some truncated)."""
    z = golden("ast_relations")
    r = _host(z["parents"], z["n_nodes"], fields=("L", "T", "L_mask", "T_mask"))
    R.assert_fields_equal(r, z, fields=("L", "T", "L_mask", "T_mask"))
    assert r.L.dtype == torch.uint8 and r.L_mask.dtype == torch.bool
    assert r.rel.shape == (12, 2, 150, 150) and r.rel.dtype == torch.uint8 and r.rel_mask.dtype == torch.uint8
    assert r.L.data_ptr() == r.rel.data_ptr() and r.T.data_ptr() == r.rel[:, 1].data_ptr()  # views, not copies
    assert r.L_mask.data_ptr() == r.rel_mask.data_ptr() and r.T_mask.data_ptr() == r.rel_mask[:, 1].data_ptr()
    assert not bool(r.status.any()) and r.num_node.tolist() == z["n_nodes"].tolist()


def test_host_backend_equals_golden_tree_pos_rows(golden):
    """tests/golden/tree_pos_ref.npz: the reference's gen_tree_positions rows, depth past 16 included."""
    z = golden("tree_pos_ref")
    trees = [z[f"par{i}"].astype(np.int32) for i in range(len([k for k in z if k.startswith("par")]))]
    parents, nn = R.pad(trees, 153)
    r = _host(parents, nn, fields=("tree_pos",))
    assert r.tree_pos.shape == (len(trees), 153, 128) and r.tree_pos.dtype == torch.float32
    for i, p in enumerate(trees):
        np.testing.assert_array_equal(r.tree_pos[i, :len(p)].numpy(), z[f"tree_pos{i}"])
        assert not bool(r.tree_pos[i, len(p):].any())
    assert not hasattr(r, "L") and not hasattr(r, "adj")  # nothing that was not asked for


def test_adj_is_the_near_band_of_golden_L(golden):
    """adj = |L - 75| <= 1 inside the n x n block, 0 outside, derived from the golden L (no |raw| >= 75 is near)."""
    z = golden("ast_relations")
    r = _host(z["parents"], z["n_nodes"], fields=("adj",))
    assert r.adj.dtype == torch.bool
    for b, n in enumerate(z["n_nodes"]):
        want = np.zeros((150, 150), bool)
        want[:n, :n] = np.abs(z["L"][b, :n, :n].astype(np.int64) - 75) <= 1
        np.testing.assert_array_equal(r.adj[b].numpy(), want)


def test_bfs_numbering_agrees_with_the_python_restatement():
    """Topological but not pre-order ids: the planes against relation_matrices + collate_relations."""
    from csa_amd.data import collate_relations, relation_matrices
    trees = [R.bfs_tree(n, seed) for n, seed in ((40, 1), (23, 2), (2, 3))]
    # not pre-order: some node with children is not followed by its first child
    par0, kids0 = trees[0]
    assert any(kids0[v] and par0[v + 1] != v for v in range(39))
    parents, nn = R.pad([t[0] for t in trees], 40)
    r = _host(parents, nn)
    for b, (par, kids) in enumerate(trees):
        rl, rt = relation_matrices(par.astype(np.int64), kids, 40)
        (L, Lm), (T, Tm) = collate_relations(rl), collate_relations(rt)
        R.assert_fields_equal(r, dict(L=L, T=T, L_mask=Lm, T_mask=Tm), b=b, fields=("L", "T", "L_mask", "T_mask"))
        want_adj = np.zeros((40, 40), bool)
        want_adj[:len(par), :len(par)] = np.abs(rl[:len(par), :len(par)]) <= 1
        np.testing.assert_array_equal(r.adj[b].numpy(), want_adj)


@pytest.mark.parametrize("edit", [{2: 2}, {2: 3}, {3: -1}, {3: -7}, {1: 2 ** 31 - 1}, {0: 0}],
                         ids=["parent=v", "parent>v", "neg-nonroot", "neg-nonroot-7", "huge-id", "root-has-parent"])
def test_malformed_inputs_raise_under_check(edit):
    from csa_amd._lib import CsaError
    parents, nn = R.pad([R.chain(6), R.star(5)], 8)
    for v, p in edit.items():
        parents[1, v] = p
    with pytest.raises(CsaError, match="pre-order"):
        _host(parents, nn, check=True)
    r = _host(parents, nn)  # without check: the empty tree and a status word, the neighbour untouched
    assert r.status.tolist() == [0, 1] and r.num_node.tolist() == [6, 5]
    R.assert_fields_equal(r, R.empty_fields(8), b=1)
    good = R.host_fields(parents[:1], nn[:1])
    R.assert_fields_equal(r, {k: v[0] for k, v in good.items()}, b=0)
    # a bad id beyond num_node is not part of the tree
    parents, nn = R.pad([R.chain(6)], 8)
    parents[0, 7] = 99
    assert _host(parents, nn, check=True).status.tolist() == [0]


def test_argument_checks():
    from csa_amd._lib import CsaError
    from csa_amd.batch_ops import ast_batch
    p, n = torch.zeros(2, 5, dtype=torch.int32), torch.tensor([1, 1])
    with pytest.raises(ValueError):
        ast_batch(p, n, fields=("L", "depth"))
    with pytest.raises(ValueError):
        ast_batch(p, n, backend="gpu")
    with pytest.raises(ValueError):
        ast_batch(p, n, max_size=6)
    with pytest.raises(ValueError):
        ast_batch(p, n[:1])
    with pytest.raises(CsaError, match="csa_ast_batch_supported"):
        ast_batch(p, n, backend="device")  # CPU tensors: no device builder, and no silent fallback when forced


def test_supported_sizes_and_arg_validation_without_gpu():
    """The size limit is the LDS budget (20 bytes of tables a node in 64 KiB); bad arguments are refused before any
    HIP call."""
    import ctypes
    from csa_amd import _lib
    L = _lib.lib()
    assert L.csa_ast_batch_supported(1) and L.csa_ast_batch_supported(150) and L.csa_ast_batch_supported(1024)
    assert L.csa_ast_batch_supported(3276) and not L.csa_ast_batch_supported(3277) and not L.csa_ast_batch_supported(0)
    assert L.csa_ast_batch(None, None) == 1
    a = _lib.AstBatchArgs(B=1, N=4)
    assert L.csa_ast_batch(ctypes.byref(a), None) == 1 and b"null pointer" in L.csa_last_error_str()
    a = _lib.AstBatchArgs(B=1, N=4000)
    assert L.csa_ast_batch(ctypes.byref(a), None) == 2
    a = _lib.AstBatchArgs(B=0, N=4)
    assert L.csa_ast_batch(ctypes.byref(a), None) == 0  # nothing to build: no launch
    a = _lib.AstBatchArgs(B=1, N=4, parents=4, num_node=4, status=4, tree_pos=8)
    assert L.csa_ast_batch(ctypes.byref(a), None) == 1 and b"misaligned" in L.csa_last_error_str()
    a = _lib.AstBatchArgs(B=1, N=4, parents=4, num_node=4, status=4, plane_sb=15)
    assert L.csa_ast_batch(ctypes.byref(a), None) == 1 and b"plane_sb" in L.csa_last_error_str()


def test_parents_only_synthetic_batch_completes_to_the_full_one():
    """synthetic_batch(planes=False) + ast_batch == synthetic_batch(), key by key, from the same RNG draws."""
    from csa_amd.data import synthetic_batch
    kw = dict(batch=5, max_size=40, seed=11, min_nodes=1, max_nodes=40, src_vocab=50, tgt_vocab=60, max_tgt_len=12)
    full = synthetic_batch(ablation_fields=True, **kw)
    slim = synthetic_batch(planes=False, **kw)
    assert "L" not in slim and "adj" not in slim and slim["parents"].shape == (5, 40) and slim["parents"].dtype == np.int32
    r = _host(slim["parents"], slim["num_node"])
    built = {f: getattr(r, f).numpy() for f in R.ALL}
    assert set(full) == (set(slim) - {"parents"}) | set(built)
    for k, v in full.items():
        np.testing.assert_array_equal(built[k] if k in built else slim[k], v, err_msg=k)
        assert (built[k] if k in built else slim[k]).dtype == v.dtype, k


def test_collate_parents_and_batch_to_device():
    """Items that store a parent array collate to the parents-only namespace; batch_to_device ships parents and
    num_node when the dict has no L."""
    from csa_amd.data import collate_parents, synthetic_batch
    from csa_amd.model import batch_to_device
    kw = dict(batch=3, max_size=20, seed=4, min_nodes=3, max_nodes=20, src_vocab=50, tgt_vocab=60, max_tgt_len=9)
    sb = synthetic_batch(planes=False, **kw)
    items = [({"src_seq": sb["src_seq"][b], "tgt_seq": sb["tgt_seq"][b], "target": sb["target"][b],
               "num_node": int(sb["num_node"][b]), "parents": sb["parents"][b, :int(sb["num_node"][b])]}, None)
             for b in range(3)]
    data, target = collate_parents(items)
    assert data.parents.dtype == torch.int32 and data.num_node.dtype == torch.int32
    np.testing.assert_array_equal(data.parents.numpy(), sb["parents"])
    np.testing.assert_array_equal(data.num_node.numpy(), sb["num_node"])
    np.testing.assert_array_equal(target.numpy(), sb["target"])
    assert not hasattr(data, "L")
    x, y = batch_to_device(sb, "cpu")
    assert not hasattr(x, "L") and torch.equal(x.parents, data.parents) and torch.equal(x.num_node, data.num_node)
    assert torch.equal(y, target)


@pytest.mark.parametrize("mode", ["pegen", "laplacian", "sequential", "treepos", "triplet"])
def test_process_data_builds_what_the_mode_reads_and_nothing_more(mode):
    """CSATrans.process_data on a parents-only batch (CPU tensors: the host backend)."""
    from types import SimpleNamespace

    from csa_amd.batch_ops import FIELDS_OF_MODE
    from csa_amd.data import synthetic_batch
    from csa_amd.model import CSATrans
    tiny = dict(src_vocab_size=50, tgt_vocab_size=60, hidden_size=64, num_heads=8, num_layers=1, sbm_layers=2,
                dim_feed_forward=128, dropout=0.2, pe_dim=0 if mode == "sequential" else 32, pegen_dim=128,
                sbm_enc_dim=512, clusters=[10, 12], full_att=False)
    m = CSATrans(**tiny, use_pegen=mode)
    kw = dict(batch=2, max_size=20, seed=4, min_nodes=3, max_nodes=20, src_vocab=50, tgt_vocab=60, max_tgt_len=9)
    sb, full = synthetic_batch(planes=False, **kw), synthetic_batch(ablation_fields=True, **kw)
    d = SimpleNamespace(src_seq=torch.from_numpy(sb["src_seq"]), tgt_seq=None, parents=torch.from_numpy(sb["parents"]),
                        num_node=torch.from_numpy(sb["num_node"]))
    m.process_data(d)
    want = set(FIELDS_OF_MODE[mode]) | ({"rel", "rel_mask"} if mode == "pegen" else set())
    assert {f for f in R.ALL + ("rel", "rel_mask") if hasattr(d, f)} == want
    for f in FIELDS_OF_MODE[mode]:
        np.testing.assert_array_equal(getattr(d, f).numpy(), full[f], err_msg=f)
