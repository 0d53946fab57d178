"""notes GRU forward and BPTT (csrc/notes_roles.hip), 64-row against 32-row panels, standalone at the train step's shapes: R = 32 B rows,
T = 15, the benchmark batch's own length-sorted row_len (synth_batch(B, 1234)), live_top / bound as that batch has them, nofill on --
the call the composites make -- and the plain entry points (every panel runs every step) next to it.
python scripts/bench_notes_panels.py [R ...]        (default 8192 16384 32768)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polyphonic_chord_texture_disentanglement_amd import functional as F_  # noqa: E402
from polyphonic_chord_texture_disentanglement_amd._lib import call, lib, ptr, stream_ptr  # noqa: E402
from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch  # noqa: E402

dev = torch.device('cuda:0')
bf = torch.bfloat16
T, H, E = 15, 512, 128
FWD = {64: 0, 32: 1 << 25}
BWD = {64: 0, 32: 1 << 17}


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def one(R):
    g = torch.Generator(device=dev).manual_seed(1)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)
    x = torch.from_numpy(synth_batch(R // 32, 1234)[0]).to(dev)
    plan = F_.live_rows(x)
    row_len, top = plan.sort['len'], plan.top.to(torch.int32).clone()
    torch.cuda.synchronize()
    rl = row_len.cpu()
    print('R=%d  live_top %d, live steps per row: mean %.2f max %d; 64-row panel steps %d, 32-row %d' % (
        R, int(top.item()), rl.float().mean().item(), int(rl.max()), int(rl[::128].repeat_interleave(2)[:(R + 63) // 64].clamp(max=int(top.item()) + 1).sum()),
        int(rl[::128].repeat_interleave(4)[:(R + 31) // 32].clamp(max=int(top.item()) + 1).sum())), flush=True)
    w_hh, w_tok, b_hh = rn(3 * H, H) / H ** 0.5, rn(3 * H, E) / H ** 0.5, rn(3 * H) * 0.1
    gc = (rn(R, 3 * H) * 0.5).to(bf).view(R, 3 * H // 16, 16).permute(1, 0, 2).contiguous()
    emb, h0 = rn(T, R, E) * 0.5, rn(R, H) * 0.5
    ext = rn(T, R, H) * 0.1
    ext *= (torch.arange(T, device=dev)[:, None] < row_len[None, :]).unsqueeze(-1)          # nothing arrives at a row's dead steps
    ext_b = ext.to(bf).view(T * R, H // 32, 32).permute(1, 0, 2).contiguous()
    del ext
    wg_h, wg_t, wt = F_.pack_mfma_b(w_hh, pairs=False), F_.pack_mfma_b(w_tok, pairs=False), F_.pack_mfma_b(w_hh.t().contiguous(), pairs=True)
    HN16 = torch.zeros(T + 1, R, H, device=dev, dtype=bf)
    gates = torch.zeros(T, 4, R, H, device=dev, dtype=bf)
    dgi, dgh, dh0 = torch.zeros(T, R, 3 * H, device=dev, dtype=bf), torch.zeros(T, R, H, device=dev, dtype=bf), torch.zeros(R, H, device=dev)
    scratch = torch.empty(lib().ptv_notes_gru_persist_scratch_elems(R), device=dev, dtype=bf)
    top_step = torch.full((1,), -1, device=dev, dtype=torch.int32)

    def fwd(rows, sorted_):
        if sorted_:
            call('ptv_notes_gru_persist_fwd_rows', ptr(wg_h), ptr(wg_t), ptr(b_hh), ptr(gc), ptr(emb), ptr(h0), ptr(HN16), ptr(gates), R,
                 T | (1 << 24) | FWD[rows], ptr(top), ptr(row_len), stream_ptr())
        else:
            call('ptv_notes_gru_persist_fwd', ptr(wg_h), ptr(wg_t), ptr(b_hh), ptr(gc), ptr(emb), ptr(h0), ptr(HN16), ptr(gates), R, T | FWD[rows], stream_ptr())

    def bwd(rows, sorted_):
        if sorted_:
            call('ptv_notes_gru_persist_bwd_rows', ptr(wt), ptr(HN16), ptr(gates), ptr(ext_b), ptr(dgi), ptr(dgh), ptr(dh0), ptr(scratch), R,
                 T | (1 << 16) | BWD[rows], ptr(top), ptr(row_len), ptr(top_step), stream_ptr())
        else:
            call('ptv_notes_gru_persist_bwd', ptr(wt), ptr(HN16), ptr(gates), ptr(ext_b), ptr(dgi), ptr(dgh), ptr(dh0), ptr(scratch), R, T | BWD[rows], None,
                 stream_ptr())

    fwd(64, False)                                                       # (every state and gate plane written once: the BPTT's operands)
    for sorted_ in (True, False):
        for name, fn in (('forward', fwd), ('BPTT', bwd)):
            t = {64: [], 32: []}
            for _ in range(3):                                           # alternating: the spread of each figure next to the difference
                for rows in (64, 32):
                    t[rows].append(timeit(lambda: fn(rows, sorted_)))
            m64, m32 = min(t[64]), min(t[32])
            print('R=%d T=%d %-7s %-22s 64 rows: %s us   32 rows: %s us   t32/t64 (best of 3) %.3f' % (
                R, T, name, 'sorted rows, row_len' if sorted_ else 'plain, every step', ' '.join('%.1f' % v for v in t[64]), ' '.join('%.1f' % v for v in t[32]),
                m32 / m64), flush=True)


for R in ([int(a) for a in sys.argv[1:]] or [8192, 16384, 32768]):
    one(R)
    torch.cuda.empty_cache()
