"""The structure-encoding ablations (use_pegen = sequential / treepos / triplet / laplacian) without a GPU: the model
builds with the reference's state_dict keys, the host builders of adj / tree_pos / triplet, and the CPU fallbacks of the
tree positional encoding and of lap_pe against fp64 and the reference's fixtures."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pe_ref

TINY = dict(src_vocab_size=50, tgt_vocab_size=60, hidden_size=64, num_heads=8, num_layers=1, sbm_layers=2,
            dim_feed_forward=128, dropout=0.2, pe_dim=32, pegen_dim=128, sbm_enc_dim=512, clusters=[10, 12],
            full_att=False)
MODES = {"sequential": ("csatrans_tiny_seq", dict(pe_dim=0)), "treepos": ("csatrans_tiny_treepos", dict(pegen_dim=256)),
         "triplet": ("csatrans_tiny_triplet", {}), "laplacian": ("csatrans_tiny_lap", {})}


def tiny(mode, **kw):
    from csa_amd.model import CSATrans
    return CSATrans(**{**TINY, **MODES[mode][1], **kw}, use_pegen=mode)


@pytest.mark.parametrize("mode", list(MODES))
def test_mode_builds_with_reference_state_keys(mode, golden):
    """Every mode constructs (use_pegen != "pegen" used to raise) with the reference's parameters and keys."""
    z = golden(MODES[mode][0])
    m = tiny(mode)
    assert sorted(m.state_dict().keys()) == list(z["state_keys"])
    assert hasattr(m, "pegen") == hasattr(m, "src_pe_embedding") == False  # noqa: E712
    assert hasattr(m.SBM, "pe") == (mode == "sequential") and hasattr(m.SBM, "pe_expand") == (mode != "sequential")


def test_deterministic_fill_reproduces_the_fixture_parameter(golden):
    """The fixtures carry no weights: the fill the tests apply leaves the reference's tree_pos_enc.p."""
    from golden_inputs import fill_params_deterministic
    m = tiny("treepos")
    fill_params_deterministic(m, 74)
    np.testing.assert_array_equal(m.tree_pos_enc.p.detach().numpy(), golden("csatrans_tiny_treepos")["p:tree_pos_enc.p"])


def test_mode_parameters():
    from csa_amd.model import CSATrans, TreePositionalEncodings
    m = tiny("treepos")
    assert isinstance(m.tree_pos_enc, TreePositionalEncodings) and m.tree_pos_enc.p.shape == (2,)
    assert (m.tree_pos_enc.depth, m.tree_pos_enc.width, m.tree_pos_enc.d_model) == (16, 8, 256)
    p = m.tree_pos_enc.p.detach()
    assert float(p.min()) >= 0.7 and float(p.max()) <= 0.999
    assert tiny("triplet").triplet_emb.weight.shape == (1246, 128)
    assert tiny("triplet", triplet_vocab_size=1505).triplet_emb.weight.shape == (1505, 128)
    with pytest.raises(ValueError):
        CSATrans(**TINY, use_pegen="cse")


def test_tree_pos_matches_reference_generator(golden):
    """tree_positions against the reference's gen_tree_positions and padding on the same trees (depth past 16
    included), exactly."""
    from csa_amd.data import tree_positions
    z = golden("tree_pos_ref")
    n_trees = len([k for k in z if k.startswith("par")])
    assert n_trees >= 6
    deep = 0
    for i in range(n_trees):
        par, ref = z[f"par{i}"], z[f"tree_pos{i}"]
        got = tree_positions(par, len(par) + 3)
        np.testing.assert_array_equal(got[:len(par)], ref)
        assert not got[len(par):].any()
        deep = max(deep, int(ref.sum(1).max()))
    assert deep == 16  # a node deeper than 16 levels keeps its last 16 steps


def test_adjacency_is_its_definition_from_relation_matrices():
    from csa_amd.data import adjacency, random_tree, relation_matrices
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 37, 150):
        par, kids = random_tree(n, rng)
        Lr, _ = relation_matrices(par, kids, 152)
        ref = np.zeros((152, 152), bool)
        ref[:n, :n] = np.isin(Lr[:n, :n], (-1.0, 0.0, 1.0))
        got = adjacency(par, 152)
        np.testing.assert_array_equal(got, ref)
        assert (got == got.T).all() and got[:n, :n].diagonal().all()


def test_synthetic_batch_ablation_fields_and_collate():
    from csa_amd.data import PAD, TRIPLET_VOCAB, collect_fn, synthetic_batch, tree_levels
    from csa_amd.model import batch_to_device
    kw = dict(max_size=20, seed=7, min_nodes=12, max_nodes=20, src_vocab=50, tgt_vocab=60, max_tgt_len=9)
    plain = synthetic_batch(3, **kw)
    sb = synthetic_batch(3, **kw, ablation_fields=True)
    assert set(sb) == set(plain) | {"adj", "tree_pos", "triplet"}
    for k in plain:  # the default output is unchanged
        np.testing.assert_array_equal(plain[k], sb[k])
    assert sb["adj"].shape == (3, 20, 20) and sb["adj"].dtype == bool
    assert sb["tree_pos"].shape == (3, 20, 128) and sb["tree_pos"].dtype == np.float32
    assert sb["triplet"].shape == (3, 20) and sb["triplet"].dtype == np.int64
    for b in range(3):
        n = int(sb["num_node"][b])
        t = sb["triplet"][b]
        assert (t[n:] == PAD).all() and (t[:n] >= 2).all() and (t[:n] < TRIPLET_VOCAB).all()
        assert t[0] == 2  # the root's triplet (0, 0, 0)
        assert not sb["adj"][b, n:].any() and not sb["adj"][b, :, n:].any() and not sb["tree_pos"][b, n:].any()
    # ids follow the documented enumeration
    par = np.array([-1, 0, 1, 1, 0, 4], np.int64)
    from csa_amd.data import triplet_ids
    depth, ci = tree_levels(par)
    assert list(depth) == [0, 1, 2, 2, 1, 2] and list(ci) == [0, 0, 0, 1, 1, 0]
    assert list(triplet_ids(par, 7)) == [2, 2 + 64, 2 + 128, 2 + 128 + 1, 2 + 64 + 1, 2 + 128 + 8, PAD]
    x, _ = batch_to_device(sb, torch.device("cpu"))
    assert x.adj.dtype == torch.uint8 and x.tree_pos.dtype == torch.float32 and x.triplet.dtype == torch.int64
    assert x.num_node.dtype == torch.int32
    assert not hasattr(batch_to_device(plain, torch.device("cpu"))[0], "adj")
    # collect_fn collates the three fields when every item has them (tree_pos rows padded to N)
    items = []
    for b in range(3):
        n = int(sb["num_node"][b])
        it = {k: sb[k][b] for k in ("src_seq", "tgt_seq", "target", "adj", "triplet")}
        it.update(L=np.zeros((20, 20), np.float32), T=np.zeros((20, 20), np.float32), num_node=n,
                  tree_pos=sb["tree_pos"][b, :n])
        items.append((it, None))
    data, _ = collect_fn(items)
    np.testing.assert_array_equal(data.adj.numpy(), sb["adj"])
    np.testing.assert_array_equal(data.tree_pos.numpy(), sb["tree_pos"])
    np.testing.assert_array_equal(data.triplet.numpy(), sb["triplet"])
    del items[1][0]["triplet"]
    assert not hasattr(collect_fn(items)[0], "adj")


@pytest.mark.parametrize("F,zero_p", [(1, False), (1, True), (2, False), (2, True)])
def test_tree_pos_cpu_fallback_matches_fp64_autograd(F, zero_p):
    """CPU tensors take the reference's torch expressions: forward to rtol 1e-6 and dp within R u sum|terms| of fp64
    autograd (pe_ref.tree_pos_reference64), p holding an exact 0.0 and values in (0.7, 0.999); at p = 0 the weights
    are 0 below depth 0 and sqrt(d_model / 2) at depth 0, with torch's pow gradients."""
    from csa_amd.model import TreePositionalEncodings
    pos, p, dout = pe_ref.tree_pos_case((2, 20), F, seed=10 * F + zero_p, binary=not zero_p, zero_p=zero_p)
    ref, dp64, bound = pe_ref.tree_pos_reference64(pos, p, dout)
    enc = TreePositionalEncodings(16, 8, F, 128 * F)
    with torch.no_grad():
        enc.p.copy_(p)
    out = enc(pos)
    assert out.shape == (2, 20, 128 * F) and out.dtype == torch.float32
    np.testing.assert_allclose(out.detach().numpy(), ref.numpy(), rtol=1e-6, atol=0)
    out.backward(dout)
    err = (enc.p.grad.double() - dp64).abs()
    print("dp error", err.tolist(), "bound", bound.tolist())
    assert bool((err <= bound).all())
    if zero_p:
        w = enc.build_weights().detach().reshape(16, 8, F)
        assert bool((w[1:, :, 0] == 0).all()) and bool((w[0, :, 0] == torch.tensor(128 * F / 2).sqrt()).all())


def test_lap_pe_cpu_fallback_matches_reference_fixture(golden):
    """The host fallback against the reference's own eigh on the same adj (csatrans_tiny_lap): eigenvalues to 1e-5,
    eigenvectors of eigenvalues isolated by a gap >= 1e-2 equal up to sign to 1e-5, the sign rule, zero padding."""
    from csa_amd.pe_ops import lap_pe
    z = golden("csatrans_tiny_lap")
    adj, nn_ = torch.from_numpy(z["adj"]), torch.from_numpy(z["num_node"])
    garbage = adj.clone()
    for b, n in enumerate(nn_):  # anything outside the n x n block is ignored
        garbage[b, n:, :] = True
        garbage[b, :, n:] = True
    r = lap_pe(garbage, nn_, 128)
    assert r.pe.shape == (2, 20, 128) and r.pe.dtype == torch.float32 and r.eigenvalues.shape == (2, 20)
    assert not bool(r.status.any())
    isolated = 0
    for b, n in enumerate(int(v) for v in nn_):
        val, vec = r.eigenvalues[b, :n].numpy(), r.pe[b, :n, :n].numpy()
        # the reference reports sort(|eigenvalues|): the same values, up to the sign of the rounded zero
        np.testing.assert_allclose(np.abs(val), z["lap_val"][b, :n], atol=1e-5, rtol=0)
        for lo, hi in pe_ref.clusters(val.astype(np.float64)):
            if hi - lo == 1:
                ref = z["lap_vec"][b, :n, lo]
                s = 1.0 if float(ref @ vec[:, lo]) > 0 else -1.0
                np.testing.assert_allclose(vec[:, lo], s * ref, atol=1e-5, rtol=0)
                isolated += 1
        pe_ref.check_sign_rule(vec)
        mask = torch.ones(20, 128, dtype=torch.bool)
        mask[:n, :n] = False
        assert not bool(r.pe[b][mask].any()) and not bool(r.eigenvalues[b, n:].any())
    assert isolated >= 4
    same = lap_pe(adj.to(torch.uint8), nn_, 128, backend="host")
    assert torch.equal(same.pe, r.pe)
    with pytest.raises(ValueError):
        lap_pe(adj, nn_, 19)
    with pytest.raises(RuntimeError):
        lap_pe(adj, nn_, 128, backend="device")  # CPU tensors: the device solver cannot run


def test_lap_pe_host_invariants_on_the_gpu_test_batch():
    """The host fallback on the batch of the GPU test meets the same invariants (it is the solver of every shape the
    kernel does not take), and that batch has what the GPU test needs: every AST with n >= 12 has at least three
    eigenvalue clusters at gap 1e-2, so the projector check there compares proper subspaces."""
    from csa_amd.pe_ops import lap_pe
    adj, nn_ = pe_ref.lap_batch()
    ref = pe_ref.lap_reference()
    counts = {int(n): len(pe_ref.clusters(ref[b][1])) for b, n in enumerate(nn_)}
    print("clusters", counts)
    assert all(c >= 3 for n, c in counts.items() if n >= 12)
    r = lap_pe(torch.from_numpy(adj.copy()), torch.from_numpy(nn_), 160)
    pe_ref.check_lap_result(r.pe.numpy(), r.eigenvalues.numpy(), adj, nn_, ref)


def test_laplacian_encode_prefers_a_precomputed_lap_pe():
    """encode takes data.lap_pe when the batch carries one and calls pe_ops.lap_pe on data.adj otherwise."""
    import csa_amd.pe_ops as pe_ops
    m = tiny("laplacian")
    seen = {}

    def fake_sbm(data, src_pe, mode):
        seen["pe"], seen["mode"] = src_pe, mode
        return torch.zeros(1), (None, None), [], [], None

    m.SBM.forward = fake_sbm
    pre = torch.randn(2, 20, 128)
    m.encode(SimpleNamespace(lap_pe=pre))
    assert seen["pe"] is pre and seen["mode"] == "laplacian"
    sb = pe_ref.lap_batch(20, (12, 20), 3)
    data = SimpleNamespace(adj=torch.from_numpy(sb[0].copy()), num_node=torch.from_numpy(sb[1]))
    m.encode(data)
    assert torch.equal(seen["pe"], pe_ops.lap_pe(data.adj, data.num_node, 128).pe)
    s = tiny("sequential")
    s.SBM.forward = fake_sbm
    s.encode(SimpleNamespace())
    assert seen["pe"] is None and seen["mode"] == "sequential"
