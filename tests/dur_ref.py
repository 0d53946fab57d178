"""Plain fp64 references (numpy, CPU) of the 5-step duration decoder -- csrc/dur.hip, csrc/dur_bwd.hip, ptv_dur_out_token and
ptv_dur_out_wgrad of csrc/misc.hip -- written from the formulas of the kernel headers and include/ptvae_hip.h ("The whole 5-step
duration GRU", "Backward of the 5-step duration GRU", "Duration head"): the oracle side of tests/test_gpu_dur_kernels.py, itself
guarded by tests/test_dur_ref_host.py against torch's float64 autograd.  Every function widens its inputs to float64.

    token_0 = <sos>;  for d in 0..4:  h_{d+1} = GRU(token_d, h_d);  est_dur_d = W_out h_{d+1} + b_out;  token_{d+1} = argmax est_dur_d

The GRU's input is one of three vectors, so W_ih token + b_ih is a table: tab0 [192] for <sos>, tab [2, 192] for the one-hot tokens
0 and 1.  Gate order r | z | n, H = 64 units each.

The second half (kp_*) evaluates the same formulas in float32 with operands rounded to bf16 where the kernels round them.  It is no
reference: its error against the fp64 functions is the yardstick that the kernels' error is held to (4x, check() of the GPU test)."""
import numpy as np

F8 = np.float64
H = 64
PART_ROWS, PART_COLS = 256, 80


def _f8(a):
    return np.asarray(a, dtype=F8)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def gate_tables(w_ih, b_ih, sos):
    """tab0 [3H] = W_ih sos + b_ih;  tab [2, 3H] = W_ih onehot(0 / 1) + b_ih  (the one-hot tokens are as wide as <sos>)"""
    w_ih, b_ih, sos = _f8(w_ih), _f8(b_ih), _f8(sos)
    return w_ih @ sos + b_ih, np.stack([w_ih[:, 0] + b_ih, w_ih[:, 1] + b_ih])


def _cell(h, gi, w_hh, b_hh):
    """one GRU step from the input part gi [M, 3H] -> r, z, n, hn = W_hn h + b_hn, h'"""
    n_h = h.shape[1]
    gh = h @ w_hh.T + b_hh
    r = _sigmoid(gi[:, :n_h] + gh[:, :n_h])
    z = _sigmoid(gi[:, n_h:2 * n_h] + gh[:, n_h:2 * n_h])
    hn = gh[:, 2 * n_h:]
    n = np.tanh(gi[:, 2 * n_h:] + r * hn)
    return r, z, n, hn, (1.0 - z) * n + z * h


def _step_input(d, idx, tab0, tab, M):
    return np.broadcast_to(tab0, (M, tab0.size)) if d == 0 else tab[idx[d - 1]]


def argmax2(est2):
    """index of the maximum of each row of [.., 2]; the first maximum wins a tie"""
    est2 = _f8(est2)
    return (est2[..., 1] > est2[..., 0]).astype(np.int64)


def dur_forward(h0, w_hh, b_hh, tab0, tab, w_out, b_out, force=None):
    """-> dict: h [5, M, H] = h_1..h_5;  gates [5, 4, M, H] = (r, z, n, hn) per step;  est_dur [M, 10];  idx [5, M] (= force if given)"""
    h0, w_hh, b_hh, tab0, tab, w_out, b_out = (_f8(a) for a in (h0, w_hh, b_hh, tab0, tab, w_out, b_out))
    M, n_h = h0.shape
    hs, gates, est = np.zeros((5, M, n_h), F8), np.zeros((5, 4, M, n_h), F8), np.zeros((M, 10), F8)
    idx = np.zeros((5, M), np.int64)
    h = h0
    for d in range(5):
        r, z, n, hn, h = _cell(h, _step_input(d, idx, tab0, tab, M), w_hh, b_hh)
        hs[d], gates[d] = h, (r, z, n, hn)
        est[:, 2 * d:2 * d + 2] = h @ w_out.T + b_out
        idx[d] = argmax2(est[:, 2 * d:2 * d + 2]) if force is None else np.asarray(force)[d]
    return dict(h=hs, gates=gates, est_dur=est, idx=idx)


def token_class(d, idx):
    """class of the token FED TO step d: 0 = <sos> (d = 0), 1 + idx[d-1] afterwards"""
    idx = np.asarray(idx)
    return np.zeros(idx.shape[1], np.int64) if d == 0 else 1 + idx[d - 1].astype(np.int64)


def dur_backward(gates, hprev, ddur, idx, w_hh, w_out):
    """BPTT of sum(est_dur * ddur) from the saved gate planes [5, 4, M, H], the states h_0..h_4 [5, M, H], ddur [M, 10], the tokens
    idx [>= 4, M] and the weights -> dh0 [M, H], S [256, 80]: rows dr | dz | dn r | dn (pre-activation gradients; dn r = the gradient
    of hn), columns 0..63 = sum over steps and rows of (row gradient) x h_{d-1}, 64..66 = sums over the rows whose step input was
    <sos> / token 0 / token 1, 67..79 zero"""
    gates, hprev, ddur, w_hh, w_out = (_f8(a) for a in (gates, hprev, ddur, w_hh, w_out))
    M, n_h = hprev.shape[1:]
    S = np.zeros((4 * n_h, PART_COLS), F8)
    carry = np.zeros((M, n_h), F8)
    for d in range(4, -1, -1):
        r, z, n, hn = gates[d]
        hp = hprev[d]
        dh = carry + ddur[:, 2 * d:2 * d + 2] @ w_out                   # into h_{d+1}: from the later steps and from est_dur_d
        da_n = dh * (1.0 - z) * (1.0 - n * n)                           # h' = (1 - z) n + z h;  n = tanh(a_n), a_n = gi_n + r hn
        da_z = dh * (hp - n) * z * (1.0 - z)                            # z = sigmoid(a_z)
        d_hn = da_n * r
        da_r = da_n * hn * r * (1.0 - r)
        A = np.concatenate([da_r, da_z, d_hn, da_n], axis=1)            # [M, 4H]
        S[:, :n_h] += A.T @ hp
        cls = token_class(d, idx)
        for k in range(3):
            S[:, n_h + k] += A[cls == k].sum(axis=0)
        carry = A[:, :3 * n_h] @ w_hh + dh * z                          # the recurrent part sees (da_r, da_z, d_hn)
    return carry, S


def rebuild_gates(hprev, idx, w_hh, b_hh, tab0, tab):
    hprev, w_hh, b_hh, tab0, tab = (_f8(a) for a in (hprev, w_hh, b_hh, tab0, tab))
    M = hprev.shape[1]
    gates = np.zeros((5, 4) + hprev.shape[1:], F8)
    for d in range(5):
        gates[d] = _cell(hprev[d], _step_input(d, np.asarray(idx), tab0, tab, M), w_hh, b_hh)[:4]
    return gates


def dur_backward_recompute(hprev, ddur, idx, w_hh, b_hh, tab0, tab, w_out):
    """the same backward with the gates of step d rebuilt from h_{d-1}"""
    return dur_backward(rebuild_gates(hprev, idx, w_hh, b_hh, tab0, tab), hprev, ddur, idx, w_hh, w_out)


def dur_finalize(S, w_ih, sos):
    """the five increments of ptv_dur_bwd_finalize: dW_hh [3H, H], db_hh [3H], db_ih [3H], dW_ih [3H, I], d sos [I].  The hidden part
    differentiates through hn (rows dr | dz | dn r), the input part through a_n (rows dr | dz | dn)"""
    S, w_ih, sos = _f8(S), _f8(w_ih), _f8(sos)
    n_h = S.shape[0] // 4
    assert sos.size >= 2                                                 # the one-hot tokens 0 and 1 are as wide as <sos>
    gh = S[:3 * n_h]
    gi = np.concatenate([S[:2 * n_h], S[3 * n_h:]])[:, n_h:n_h + 3]     # [3H, 3]: per token class
    d_wih = np.outer(gi[:, 0], sos)                                     # <sos> steps: the token is sos
    d_wih[:, 0] += gi[:, 1]                                             # token 0 = e_0
    d_wih[:, 1] += gi[:, 2]                                             # token 1 = e_1
    return gh[:, :n_h].copy(), gh[:, n_h:n_h + 3].sum(1), gi.sum(1), d_wih, gi[:, 0] @ w_ih


def dur_out_token(h, w_out, b_out):
    """est [rows, 2] = W_out h + b_out, idx [rows] = its argmax"""
    est = _f8(h) @ _f8(w_out).T + _f8(b_out)
    return est, argmax2(est)


def dur_out_wgrad(ddur, hplanes):
    """gw [2, H] = sum_d sum_m ddur[m, 2d + c] h_{d+1}[m, :], hplanes [5, M, H] = h_1..h_5.  A row whose two gradients of a step are
    both zero is EXCLUDED from that step, never multiplied by zero: its state may hold anything"""
    ddur, hplanes = _f8(ddur), _f8(hplanes)
    gw = np.zeros((2, hplanes.shape[2]), F8)
    for d in range(5):
        g = ddur[:, 2 * d:2 * d + 2]
        live = (g != 0).any(axis=1)
        gw += g[live].T @ hplanes[d][live]
    return gw


# ================================================================================================ the kernels' own precision
F4 = np.float32


def _f4(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F4))


def bf16_round(a):
    """fp32 -> the nearest bf16 (ties to even) -> fp32; finite inputs"""
    u = _f4(a).view(np.uint32)
    return ((u + (((u >> 16) & 1) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)).view(F4)


def is_bf16(a):
    return np.array_equal(bf16_round(a), _f4(a))


def _sigmoid4(x):
    return (F4(1) / (F4(1) + np.exp(-x))).astype(F4)


def _kp_cell(h, gi, w16, b_hh):
    """fp32, with the state that feeds h . W_hh^T and W_hh rounded to bf16 (csrc/dur.hip: "mirrored as bf16 into a per-wave LDS tile
    that feeds the next step's MFMA A operand", "W_hh (bf16, 192 x 64)"); the z h term of the update keeps the fp32 state"""
    n_h = h.shape[1]
    gh = bf16_round(h) @ w16.T
    r = _sigmoid4(gi[:, :n_h] + gh[:, :n_h] + b_hh[:n_h])
    z = _sigmoid4(gi[:, n_h:2 * n_h] + gh[:, n_h:2 * n_h] + b_hh[n_h:2 * n_h])
    hn = gh[:, 2 * n_h:] + b_hh[2 * n_h:]
    n = np.tanh(gi[:, 2 * n_h:] + r * hn).astype(F4)
    return r, z, n, hn, ((F4(1) - z) * n + z * h).astype(F4)


def kp_forward(h0, w_hh, b_hh, tab0, tab, w_out, b_out, idx):
    """dur_forward in the forward kernel's precision, the tokens given"""
    h0, w_hh, b_hh, tab0, tab, w_out, b_out = (_f4(a) for a in (h0, w_hh, b_hh, tab0, tab, w_out, b_out))
    w16 = bf16_round(w_hh)
    M, n_h = h0.shape
    hs, gates, est = np.zeros((5, M, n_h), F4), np.zeros((5, 4, M, n_h), F4), np.zeros((M, 10), F4)
    h = h0
    for d in range(5):
        r, z, n, hn, h = _kp_cell(h, _step_input(d, np.asarray(idx), tab0, tab, M), w16, b_hh)
        hs[d], gates[d] = h, (r, z, n, hn)
        est[:, 2 * d:2 * d + 2] = h @ w_out.T + b_out
    return dict(h=hs, gates=gates, est_dur=est)


def kp_backward(gates, hprev, ddur, idx, w_hh, w_out, b_hh=None, tab0=None, tab=None):
    """dur_backward in the backward kernel's precision: fp32, with dr, dz, dnr, dn rounded to bf16 before the carry product and the
    partial products, h rounded to bf16 before the partial products, W_hh in bf16 (csrc/dur_bwd.hip: "dgh_d . W_hh ... is 24
    v_mfma_f32_16x16x32_bf16", "transposed copies (K = block rows) for the parameter-gradient products").  gates None: rebuilt as the
    forward kernel builds them, from h_{d-1} rounded to bf16"""
    hprev, ddur, w_hh, w_out = (_f4(a) for a in (hprev, ddur, w_hh, w_out))
    w16 = bf16_round(w_hh)
    M, n_h = hprev.shape[1:]
    S = np.zeros((4 * n_h, PART_COLS), F4)
    carry = np.zeros((M, n_h), F4)
    for d in range(4, -1, -1):
        hp = hprev[d]
        if gates is None:
            r, z, n, hn = _kp_cell(hp, _step_input(d, np.asarray(idx), _f4(tab0), _f4(tab), M), w16, _f4(b_hh))[:4]
        else:
            r, z, n, hn = _f4(gates)[d]
        dh = carry + ddur[:, 2 * d:2 * d + 1] * w_out[0] + ddur[:, 2 * d + 1:2 * d + 2] * w_out[1]
        da_n = dh * (F4(1) - z) * (F4(1) - n * n)
        da_z = dh * (hp - n) * z * (F4(1) - z)
        A = bf16_round(np.concatenate([da_n * hn * r * (F4(1) - r), da_z, da_n * r, da_n], axis=1))
        S[:, :n_h] += A.T @ bf16_round(hp)
        cls = token_class(d, idx)
        for k in range(3):
            S[:, n_h + k] += A[cls == k].sum(axis=0, dtype=F4)
        carry = (A[:, :3 * n_h] @ w16 + dh * z).astype(F4)
    return carry, S


def kp_finalize(S, w_ih, sos, start):
    """start + dur_finalize in fp32; start: the five buffers the kernel adds into"""
    S, w_ih, sos = _f4(S), _f4(w_ih), _f4(sos)
    n_h = S.shape[0] // 4
    gh = S[:3 * n_h]
    gi = np.concatenate([S[:2 * n_h], S[3 * n_h:]])[:, n_h:n_h + 3]
    d_wih = (gi[:, :1] * sos[None, :]).astype(F4)
    d_wih[:, 0] += gi[:, 1]
    d_wih[:, 1] += gi[:, 2]
    inc = (gh[:, :n_h], gh[:, n_h] + gh[:, n_h + 1] + gh[:, n_h + 2], gi[:, 0] + gi[:, 1] + gi[:, 2], d_wih,
           (gi[:, :1] * w_ih).sum(axis=0, dtype=F4))
    return tuple((_f4(s) + i).astype(F4) for s, i in zip(start, inc))


def kp_out_token(h, w_out, b_out):
    return (_f4(h) @ _f4(w_out).T + _f4(b_out)).astype(F4)


def kp_out_wgrad(ddur, hplanes16, start):
    """start + dur_out_wgrad in fp32 on the bf16 states (given as fp32 values)"""
    ddur, hp = _f4(ddur), _f4(hplanes16)
    gw = np.zeros((2, hp.shape[2]), F4)
    for d in range(5):
        g = ddur[:, 2 * d:2 * d + 2]
        live = (g != 0).any(axis=1)
        gw += g[live].T @ hp[d][live]
    return (_f4(start) + gw).astype(F4)
