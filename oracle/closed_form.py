"""ORACLE (test infrastructure only): closed-form fp64 forward/backward of SBM attention.

This is the math the HIP kernels implement (flash-style: no N x N intermediate is needed
beyond one tile), written out explicitly so it can be checked against the reference's
autograd (oracle/sbm_ref.py, itself pinned to tests/golden). Reference: module/sbm_attn.py:32-66,
module/STE.py:8-19.

Forward, per (b,h), query row i, key j (M keys, pad keys have mask=1):
    C   = layer.weight.reshape(H,k,d)[h];  S = softmax_{k^2}(C C^T)               (sbm_attn.py:37-39)
    Qh  = sigmoid(MLP(Q) C^T),  Kh = sigmoid(MLP(K) C^T),  T = Kh S^T (T_j = S Kh_j)  (:41-53)
    expA_ij = Qh_i . T_j ;  A_ij = [u_ij < clamp(expA_ij, .01, .99)]                 (:55, STE.py:10-15)
    e_ij = exp(s_ij - m_i), s = QK^T/sqrt(d) (pad keys -> e=0);  Z_i = sum_j e_ij
    Zg_i = sum_j e_ij A_ij ;  n_i = Zg_i / Z_i ;  D_i = max(n_i, 1e-12)                (:59-62)
    attn_ij = e_ij A_ij / (Z_i D_i);  X_i = sum_j attn_ij r_ij V_j  (r = dropout mult)  (:63)
    sparsity_h = sum_{b,i,j} A_ij / (B N M)                                           (:64)
Backward (F.normalize's L1 norm has grad sign(M), sign(0)=0; clamp_min passes iff n>=eps):
    gamma_i = dX_i . X_i   (= sum_j dattn_ij attn_ij)
    dattn_ij = r_ij (dX_i . V_j) (+ grad of the returned attn map)
    dM_ij = (dattn_ij - [n_i>=eps][M_ij>0] gamma_i) / D_i
    dP_ij = dM_ij A_ij ;  rho_i = sum_j P_ij dP_ij = (n_i>=eps ? 0 : gamma_i)
    ds_ij = P_ij (dP_ij - rho_i) / sqrt(d)  -> dQ += ds K, dK += ds^T Q
    dA_ij = dM_ij P_ij + dsparsity_h/(B N M) (+ grad of the returned graph)
    G_ij  = hardtanh(A_ij dA_ij)                                                      (STE.py:19)
    dQh = G T ;  dT = G^T Qh ;  dKh = dT S ;  dS += dT^T Kh (summed over b)
    then sigmoid', C^T, MLP backward; dS -> softmax_{k^2} backward -> dC += (dD + dD^T) C.
Upstream gradients of the returned maps (sbm_attn.py:66): dgraph adds to dA, dattn (the gradient of the
PRE-dropout attn map) adds to dattn_ij without the dropout multiplier and sum_j dattn_ij attn_ij to gamma_i.
The kernels fold dropout's 1/(1-p) into the row constant 1/D_i (k_attn_rowprep rec[1]) and therefore scale
the upstream dattn by (1 - p) (csa_sbm.hip k_attn_bwd_qr / k_attn_bwd_kv, the DG branch): the same sum.

bf16=True follows the DESIGN of the CSA_DTYPE_BF16 kernels, rounding exactly the operands their bf16 MFMAs
round (audited against csrc/csa_sbm.hip; the kernel site of each rounding point is named where it is
emulated). dtype=torch.float32 runs the same code in fp32 arithmetic (emulation_budget()).
"""
import math

import torch

EPS = 1e-12


TIE_FACTOR = 8.0 * 2.0 ** -24  # a ReLU pre-activation within this multiple of its fp32 error bound is a tie


def _ident(t):
    return t


def _bf16_round(t):
    """Round to bf16 (RNE) and back: the operand rounding of a bf16-MFMA contraction (csa_common.hpp pack8,
    v_cvt_pk_bf16_f32). The kernels round an fp32 value, so the value passes through fp32 first."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def _relu_layer(xin, Wl, bl, keep, R, ov):
    """h = drop(relu(R(x) R(W)^T + b)) with the pre-activation z and its fp32 error bound |R(x)| |R(W)|^T + |b|
    (every term of the dot product at its magnitude: the first-order fp32 error of z is at most d 2^-24 bound).
    ov: {index tuple: bool} forces the relu mask of the named elements (the ReLU-tie rule); a bool tensor of z's
    shape forces the whole mask (a run in other arithmetic on the same masks)."""
    z = R(xin) @ R(Wl).T + bl
    bound = R(xin).abs() @ R(Wl).abs().T + bl.abs()
    m = z > 0
    if isinstance(ov, torch.Tensor):
        m = ov.to(torch.bool)
    elif ov:
        m = m.clone()
        for idx, val in ov.items():
            m[tuple(idx)] = bool(val)
    h = z * m.to(z.dtype)
    if keep is not None:
        h = h * keep
    return h, m, z, bound


def _mlp_fwd(x, W, keep, R=_ident, ov=(None, None)):
    """Returns (out, [inputs of each Linear], [relu masks], [(z, bound, live) of each relu layer]). R rounds the
    operands of each x W^T product (bf16 emulation: frag_chain<BF16> packs both operands, csa_sbm.hip:227-232);
    the bias is added exactly, as the kernels do (add_bias, one fp32 MFMA K-step); dropout multiplies before the
    relu (DropWords::apply), which is relu(z) * keep for keep >= 0."""
    W0, b0, W1, b1, W2, b2 = W
    k0 = keep[0] if keep is not None else None
    k1 = keep[1] if keep is not None else None
    h1, m0, z0, bd0 = _relu_layer(x, W0, b0, k0, R, ov[0])
    h2, m1, z1, bd1 = _relu_layer(h1, W1, b1, k1, R, ov[1])
    out = R(h2) @ R(W2).T + b2
    live = lambda kk, z: torch.ones_like(z, dtype=torch.bool) if kk is None else kk > 0
    return out, (x, h1, h2), (m0, m1), ((z0, bd0, live(k0, z0)), (z1, bd1, live(k1, z1)))


def _mlp_bwd(dout, W, acts, masks, keep, R=_ident):
    """k_proj_bwd_s<D, BF>: the W^T chains and the dW outer products round both operands (mm_acc_f<.., BF>,
    outer_stage_s<D, BF>; h1 / h2 are read back as the bf16 the forward saved, store_act_lds_bf, which is R(h)
    again); the bias sums (own_rowsum) and the relu / dropout step read the unrounded fp32 gradient."""
    W0, b0, W1, b1, W2, b2 = W
    x, h1, h2 = acts
    m0, m1 = (m.to(dout.dtype) for m in masks)
    g = {}
    g["proj.6.weight"] = torch.einsum("...o,...i->oi", R(dout), R(h2))
    g["proj.6.bias"] = dout.reshape(-1, dout.shape[-1]).sum(0)
    dh2 = R(dout) @ R(W2)
    dz1 = dh2 * m1
    if keep is not None and keep[1] is not None:
        dz1 = dz1 * keep[1]
    g["proj.3.weight"] = torch.einsum("...o,...i->oi", R(dz1), R(h1))
    g["proj.3.bias"] = dz1.reshape(-1, dz1.shape[-1]).sum(0)
    dh1 = R(dz1) @ R(W1)
    dz0 = dh1 * m0
    if keep is not None and keep[0] is not None:
        dz0 = dz0 * keep[0]
    g["proj.0.weight"] = torch.einsum("...o,...i->oi", R(dz0), R(x))
    g["proj.0.bias"] = dz0.reshape(-1, dz0.shape[-1]).sum(0)
    dx = R(dz0) @ R(W0)
    return dx, g


def _pv_online(s, A, keep01, V, R):
    """sum_j w_ij V_j of k_attn_fwd<BF = true> before the row scale: the kernel walks the 32-key tiles in
    ascending order with an online softmax, so the weight it rounds to bf16 for the PV MFMA is
    exp(s_ij - m_t) A_ij keep_ij with m_t the row's running maximum after tile t (csa_sbm.hip:1286-1311:
    m_use, w[r], pack8(&w[0])), keep a 0 / 1 flag (dropout's 1 / (1 - p) is applied once per row afterwards,
    :1360), and earlier tiles are rescaled in fp32 by exp(m_t - m_final). Returned relative to the row's
    final maximum (what Z is relative to). Tiles with every key masked leave the running maximum alone."""
    B, H, N, M = s.shape
    NT = (M + 31) // 32
    pad = NT * 32 - M
    padf = lambda t, v: torch.nn.functional.pad(t, (0, pad), value=v)
    st = padf(s, float("-inf")).reshape(B, H, N, NT, 32)
    run = torch.cummax(st.max(-1).values, -1).values
    m_use = torch.where(torch.isinf(run), torch.zeros_like(run), run)  # an all-masked prefix stays finite
    e = torch.exp(st - m_use[..., None])
    w = R(e * padf(A, 0.0).reshape(B, H, N, NT, 32) * padf(keep01, 0.0).reshape(B, H, N, NT, 32))
    w = w * torch.exp(m_use - m_use[..., -1:])[..., None]
    return w.reshape(B, H, N, NT * 32)[..., :M] @ R(V)


def _attn_core(Q, K, V, mask, A, dX, r, dattn_up, R, bf16, attn_p):
    """Masked softmax x graph x dropout attention, forward and the backward up to ds and dM (shared by the SBM
    and the dense entry points). r: pre-scaled dropout multiplier (0 or 1 / (1 - p)) or None; attn_p: the dropout
    probability behind r (the bf16 forward applies 1 / (1 - p) once per row, in fp32 like the kernel)."""
    d = Q.shape[-1]
    # k_attn_fwd:1249, k_attn_bwd_qr:1712, k_attn_bwd_kv:2287 -- pack8 of both the K rows and the q rows
    s = (R(Q) @ R(K).transpose(-1, -2)) / math.sqrt(d)
    s = s.masked_fill(mask[:, None, None, :] == 1, float("-inf"))
    mrow = s.max(-1, keepdim=True).values
    e = torch.exp(s - mrow)
    Z = e.sum(-1, keepdim=True)
    P = e / Z
    Mm = P * A
    n = Mm.sum(-1, keepdim=True)
    Dn = n.clamp_min(EPS)
    attn = Mm / Dn
    dscale = 1.0
    if r is None:
        r = torch.ones_like(attn)
    elif bf16:
        if attn_p is None:
            raise ValueError("bf16=True with attn_keep needs attn_p (the row scale 1 / (1 - p) is applied apart)")
        dscale = float(torch.tensor(1.0, dtype=torch.float32) / (1.0 - torch.tensor(attn_p, dtype=torch.float32)))
    if bf16:
        X = _pv_online(s, A, (r > 0).to(s.dtype), V, R) * (dscale / (Z * Dn))
    else:
        X = (attn * r) @ V
    c = dict(s=s, mrow=mrow, Z=Z, P=P, Mm=Mm, n=n, Dn=Dn, attn=attn, X=X)
    # k_attn_bwd_kv:2351,2387-2393 -- awv = P rec[1] for a sampled, kept element (= attn r), pack8(awv), pack8(xc)
    c["dV"] = R(attn * r).transpose(-1, -2) @ R(dX)
    # k_attn_bwd_qr:1715 / k_attn_bwd_kv:2290 -- dP = dX V^T, both packed
    dattn = (R(dX) @ R(V).transpose(-1, -2)) * r
    gamma = (dX * X).sum(-1, keepdim=True)  # k_attn_rowprep: fp32 on the stored X
    if dattn_up is not None:
        dattn = dattn + dattn_up
        amap = attn
        if bf16:
            # k_attn_gx recomputes attn "like k_maps" (csa_sbm.hip:1495-1505): fp32 MFMA on the UNROUNDED q, k
            # with the bf16 forward's lse and 1 / D -- the map bf16 mode returns, not the bf16-score one
            sx = ((Q @ K.transpose(-1, -2)) / math.sqrt(d)).masked_fill(mask[:, None, None, :] == 1, float("-inf"))
            amap = torch.exp(sx - (mrow + torch.log(Z))) * A / Dn
        gamma = gamma + (dattn_up * amap).sum(-1, keepdim=True)
    big = (n >= EPS).to(s.dtype)
    dM = (dattn - big * (Mm > 0).to(s.dtype) * gamma) / Dn
    dP = dM * A
    rho = (1 - big) * gamma
    ds = P * (dP - rho) / math.sqrt(d)
    ds = torch.nan_to_num(ds)  # pad keys: P == 0
    # k_attn_bwd_qr:1785-1789 (dQ), k_attn_bwd_kv:2387-2394 (dK): pack8(dsv) with the 1/sqrt(d) inside
    c["dQ"] = R(ds) @ R(K)
    c["dK"] = R(ds).transpose(-1, -2) @ R(Q)
    c["dM"] = dM
    return c


def sbm_fwd_bwd(Q, K, V, mask, params, u, num_clusters, dX, dsparsity, attn_keep=None, proj_keep=None,
                graph_override=None, bf16=False, dgraph=None, dattn=None, relu_override=None, dtype=torch.float64,
                attn_p=None):
    """Closed-form forward + backward in `dtype` arithmetic (fp64). Returns (outputs dict, grads dict).

    bf16=True: an ideal CSA_DTYPE_BF16 implementation -- the operands of every contraction the bf16 mode
    runs on bf16 MFMA are rounded to bf16 where the kernels round them (QK^T, dX V^T, PV with the unnormalised
    0/1-dropout weights of the online softmax, dV, dQ, dK, the three MLP layers and .C^T forward, C^T dZ, the
    W^T chains and the dW outer products backward; dC reads the projection output p as the bf16 mode saves it,
    rounded to bf16), everything else (accumulation, biases, softmax, sampling, expA, T, dQh, dT, dS, dZ) exact.
    dgraph / dattn: upstream gradients of the returned graph / (pre-dropout) attn maps.
    relu_override: {"q0" | "q1" | "k0" | "k1": {(b, h, row, feature): bool}} forces relu masks of the Q / K MLP's
    first / second layer; a bool tensor instead of the inner dict forces that layer's whole mask (out["relu_masks"]
    of another run). attn_p: the probability behind attn_keep (needed with bf16=True). The outputs carry "relu_pre" (z, bound, live per layer) and "relu_ties": the
    [(layer key, index, |z| / bound)] with |z| < TIE_FACTOR * bound (dropped elements excluded)."""
    R = _bf16_round if bf16 else _ident
    f = lambda t: None if t is None else t.detach().to(dtype)
    Q, K, V, mask, u, dX, dsparsity, dgraph, dattn = map(f, (Q, K, V, mask, u, dX, dsparsity, dgraph, dattn))
    attn_keep = f(attn_keep)
    pk = {k: f(v) for k, v in (proj_keep or {}).items()}
    ov = relu_override or {}
    W = tuple(f(params[k]) for k in ("proj.0.weight", "proj.0.bias", "proj.3.weight", "proj.3.bias",
                                      "proj.6.weight", "proj.6.bias"))
    B, H, N, d = Q.shape
    M = V.shape[2]
    k = num_clusters
    C = f(params["layer.weight"]).reshape(H, k, d)
    D2 = C @ C.transpose(-1, -2)
    S = torch.softmax(D2.reshape(H, k * k), -1).reshape(H, k, k)
    Qp, qacts, qmasks, qpre = _mlp_fwd(Q, W, (pk.get("q0"), pk.get("q1")), R, (ov.get("q0"), ov.get("q1")))
    Kp, kacts, kmasks, kpre = _mlp_fwd(K, W, (pk.get("k0"), pk.get("k1")), R, (ov.get("k0"), ov.get("k1")))
    relu_pre = {"q0": qpre[0], "q1": qpre[1], "k0": kpre[0], "k1": kpre[1]}
    ties = []
    for key, (z, bd, live) in relu_pre.items():
        hit = (z.abs() < TIE_FACTOR * bd) & live
        for idx in hit.nonzero().tolist():
            ties.append((key, tuple(idx), float(z[tuple(idx)].abs() / bd[tuple(idx)])))
    # cluster_hat<.., BF>: frag_chain packs C and the projection output
    Qh = torch.sigmoid(R(Qp) @ R(C).transpose(-1, -2).unsqueeze(0))
    Kh = torch.sigmoid(R(Kp) @ R(C).transpose(-1, -2).unsqueeze(0))
    T = Kh @ S.transpose(-1, -2).unsqueeze(0)  # T_j = S Kh_j
    expA = Qh @ T.transpose(-1, -2)
    if graph_override is not None:
        A = f(graph_override)
    else:
        A = (u < expA.clamp(0.01, 0.99)).to(dtype)
    c = _attn_core(Q, K, V, mask, A, dX, attn_keep, dattn, R, bf16, attn_p)
    P, n, X, dM = c["P"], c["n"], c["X"], c["dM"]
    sparsity = A.sum((0, 2, 3)) / (B * N * M)
    out = dict(X=X, sparsity=sparsity, graph=A, attn=c["attn"], expA=expA, Qhat=Qh, Khat=Kh, T=T, S=S,
               rowmax=c["mrow"][..., 0], Z=c["Z"][..., 0], n=n[..., 0], relu_pre=relu_pre, relu_ties=ties,
               relu_masks={"q0": qmasks[0], "q1": qmasks[1], "k0": kmasks[0], "k1": kmasks[1]})

    g = {}
    g["V"] = c["dV"]
    dA = dM * P + (dsparsity / (B * N * M)).view(1, H, 1, 1)
    if dgraph is not None:
        dA = dA + dgraph
    G = (A * dA).clamp(-1, 1)
    dQh = G @ T
    dT = G.transpose(-1, -2) @ Qh
    dKh = dT @ S  # T_j = S Kh_j  ->  dKh_j = S^T dT_j
    dS = torch.einsum("bhja,bhjc->hac", dT, Kh)
    dZq = dQh * Qh * (1 - Qh)
    dZk = dKh * Kh * (1 - Kh)
    # k_proj_bwd_s:3163 mm_acc_f<.., BF>: dp = C^T dZ with both operands packed
    dQp = R(dZq) @ R(C).unsqueeze(0)
    dKp = R(dZk) @ R(C).unsqueeze(0)
    # k_proj_bwd_s:3169-3172: fp32 16x16x4 MFMA of the fp32 dZ with po widened from its saved bf16 (widen_act_bf)
    dC = torch.einsum("bhnk,bhnd->hkd", dZq, R(Qp)) + torch.einsum("bhnk,bhnd->hkd", dZk, R(Kp))
    dD = S * (dS - (S * dS).sum((-1, -2), keepdim=True))
    dC = dC + (dD + dD.transpose(-1, -2)) @ C
    dQm, gq = _mlp_bwd(dQp, W, qacts, qmasks, (pk.get("q0"), pk.get("q1")), R)
    dKm, gk = _mlp_bwd(dKp, W, kacts, kmasks, (pk.get("k0"), pk.get("k1")), R)
    g["Q"] = c["dQ"] + dQm
    g["K"] = c["dK"] + dKm
    g["layer.weight"] = dC.reshape(H * k, d)
    for key in gq:
        g[key] = gq[key] + gk[key]
    g["_G"] = G
    g["_dQhat"] = dQh
    g["_dT"] = dT
    g["_dS"] = dS
    return out, g


def dense_fwd_bwd(Q, K, V, mask, dX, attn_keep=None, dattn=None, bf16=False, dtype=torch.float64, attn_p=None):
    """FullAttention (sbm_attn.py:77-87; the kernels' DENSE instantiations): the A == 1, no-cluster subset of
    sbm_fwd_bwd. Returns (dict(X, attn), dict(Q, K, V))."""
    R = _bf16_round if bf16 else _ident
    f = lambda t: None if t is None else t.detach().to(dtype)
    Q, K, V, mask, dX, attn_keep, dattn = map(f, (Q, K, V, mask, dX, attn_keep, dattn))
    A = torch.ones(Q.shape[0], Q.shape[1], Q.shape[2], K.shape[2], dtype=dtype)
    c = _attn_core(Q, K, V, mask, A, dX, attn_keep, dattn, R, bf16, attn_p)
    return dict(X=c["X"], attn=c["attn"]), dict(Q=c["dQ"], K=c["dK"], V=c["dV"])


def elem_metric(got, ref):
    """The smallest tol with |got - ref| <= tol |ref| + tol max|ref| element-wise."""
    got, ref = got.double(), ref.double()
    scale = max(float(ref.abs().max()), 1e-30)
    return float(((got - ref).abs() / (ref.abs() + scale)).max())


def fro_metric(got, ref):
    got, ref = got.double(), ref.double()
    return float(torch.linalg.norm(got - ref) / max(float(torch.linalg.norm(ref)), 1e-30))


def emulation_budget(case):
    """How far fp32 accumulation, and the bf16 rounding flips it causes, move an honest bf16-operand
    implementation: {tensor: (elem_metric, relative Frobenius error)} (expA: (largest absolute difference, relative
    Frobenius error)) between the bf16=True emulation in fp64
    arithmetic and the SAME code in fp32 arithmetic, on the same graph and dropout masks. `case` holds the
    keyword arguments of sbm_fwd_bwd (with "params") or of dense_fwd_bwd (without). Oracle only: no kernel runs."""
    kw = dict(case)
    kw.pop("bf16", None)
    kw.pop("dtype", None)
    dense = "params" not in kw
    fn = dense_fwd_bwd if dense else sbm_fwd_bwd
    o64, g64 = fn(**kw, bf16=True, dtype=torch.float64)
    if not dense:
        kw["graph_override"] = o64["graph"]
        # a ReLU tie element takes the fp64 run's side in the fp32 run too: a tie is exempted by the tie rule and must
        # not leak into the budget as a whole-row gradient difference (the flips that a flipped bf16 rounding of an
        # activation causes away from the kink stay in: an honest kernel has them)
        ov = dict(kw.get("relu_override") or {})
        for key, idx, _ in o64["relu_ties"]:
            ov.setdefault(key, {})
            if not isinstance(ov[key], torch.Tensor):
                ov[key] = {**ov[key], idx: bool(o64["relu_masks"][key][idx])}
        kw["relu_override"] = ov
    o32, g32 = fn(**kw, bf16=True, dtype=torch.float32)
    res = {"X": (elem_metric(o32["X"], o64["X"]), fro_metric(o32["X"], o64["X"]))}
    if not dense:  # the sampling probabilities: largest absolute move (the graph compares u with clamp(expA))
        res["expA"] = (float((o32["expA"].double() - o64["expA"]).abs().max()), fro_metric(o32["expA"], o64["expA"]))
    for name in g64:
        if not name.startswith("_"):
            res[name] = (elem_metric(g32[name], g64[name]), fro_metric(g32[name], g64[name]))
    return res
