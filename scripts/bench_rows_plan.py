"""The row plan and the mapped products of the B = 512 step, standalone (R = 16384 decoder rows, the synthetic batch's note counts):
ptv_rows_plan against ptv_rows_by_length + ptv_gather_rows + ptv_rows_seg_counts, and the dNS / dtok products of ptv_decoder_tf_bwd storing
through the permutation (ptv_gemm_mtop_seg_map) against the unmapped products plus the scatter passes they replace.  Best of 20, events
around the calls of one variant (launch gaps between them included, as on the decoder's chain)."""
import sys
import torch
sys.path.insert(0, '.')
from polyphonic_chord_texture_disentanglement_amd._lib import call, ptr, stream_ptr
from polyphonic_chord_texture_disentanglement_amd.synthetic import synth_batch

dev = torch.device('cuda:0')
B = 512; R = 32 * B; T = 15; M = T * R
E, Hn, Ht = 128, 512, 1024
bf = torch.bfloat16
i32 = dict(device=dev, dtype=torch.int32)
x = torch.from_numpy(synth_batch(B, 99)[0]).to(dev)
row_live = torch.zeros(R, **i32)
pt = torch.empty(B * 480, **i32); dt = torch.empty(B * 2400, **i32); cnt = torch.zeros(3, **i32)
call('ptv_pianotree_targets_rows', ptr(x), B, 1, ptr(pt), ptr(dt), ptr(cnt), ptr(row_live), stream_ptr())
perm, len_s, seg = torch.empty(R, **i32), torch.empty(R, **i32), torch.empty(T, **i32)
perm2, len2, seg2 = torch.empty(R, **i32), torch.empty(R, **i32), torch.empty(T, **i32)


def three_calls():
    call('ptv_rows_by_length', ptr(row_live), ptr(perm), R, 15, stream_ptr())
    call('ptv_gather_rows', ptr(len_s), ptr(row_live), ptr(perm), R, 1, 0, 0, 1, stream_ptr())
    call('ptv_rows_seg_counts', ptr(len_s), R, T, ptr(seg), stream_ptr())


def plan():
    call('ptv_rows_plan', ptr(row_live), R, 15, T, ptr(perm2), ptr(len2), ptr(seg2), stream_ptr())


def best_us(f, n=20):
    best = 1e9
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best * 1e3


three_calls(); plan(); torch.cuda.synchronize()
assert torch.equal(perm, perm2) and torch.equal(len_s, len2) and torch.equal(seg, seg2)
top = cnt[2:3].clone()
print('live note steps', int(top) + 1, 'seg_n', seg.tolist())
print('%-64s %8.1f us' % ('ptv_rows_by_length + ptv_gather_rows + ptv_rows_seg_counts', best_us(three_calls)))
print('%-64s %8.1f us' % ('ptv_rows_by_length alone', best_us(lambda: call('ptv_rows_by_length', ptr(row_live), ptr(perm), R, 15, stream_ptr()))))
print('%-64s %8.1f us' % ('ptv_rows_plan', best_us(plan)))

g = torch.Generator(device=dev).manual_seed(1)
dgi = (0.1 * torch.randn(M, 3 * Hn, device=dev, generator=g)).to(bf)
live = (torch.arange(R, device=dev)[None, :] < seg[:, None]) & (torch.arange(T, device=dev)[:, None] <= top)      # [T, R] in sorted order
dgi.view(T, R, 3 * Hn)[~live] = 0                                  # the dead rows of A are zero, as the BPTT leaves them declared
w = (0.1 * torch.randn(Ht + E, 3 * Hn, device=dev, generator=g)).to(bf)
dGC = 0.1 * torch.randn(R, 3 * Hn, device=dev, generator=g); dHN0 = 0.1 * torch.randn(R, Hn, device=dev, generator=g)
w2 = (0.1 * torch.randn(Ht, Hn, device=dev, generator=g)).to(bf)
dtok_s, dtok, dtok_m = (torch.empty(T, R, E, device=dev) for _ in range(3))
dns_s, dns, dns_m = (torch.empty(R, Ht, device=dev) for _ in range(3))
A16, B16 = 1, 2


def tok(C, rows):
    call('ptv_gemm_mtop_seg_map', 1, 0, 0, M, E, 3 * Hn, ptr(dgi), 3 * Hn, w.data_ptr() + 2 * Ht * 3 * Hn, 3 * Hn, ptr(C), E, None, 1.0, 0, 0, 0, A16 | B16,
         ptr(top), R, ptr(seg), R, T, ptr(rows), R, stream_ptr())


def ns(C, rows):
    call('ptv_gemm_mtop_seg_map', 1, 0, 0, R, Ht, 3 * Hn, ptr(dGC), 3 * Hn, ptr(w), 3 * Hn, ptr(C), Ht, None, 1.0, 0, 0, 0, B16, None, 0, None, 0, 0,
         ptr(rows), R, stream_ptr())
    call('ptv_gemm_mtop_seg_map', 1, 0, 0, R, Ht, Hn, ptr(dHN0), Hn, ptr(w2), Hn, ptr(C), Ht, None, 1.0, 1, 0, 0, B16, None, 0, None, 0, 0,
         ptr(rows), R, stream_ptr())


def tok_old():
    tok(dtok_s, None)
    call('ptv_scatter_rows_seg', ptr(dtok), ptr(dtok_s), ptr(perm), R, E, R * E, R * E, T, ptr(seg), stream_ptr())


def ns_old():
    ns(dns_s, None)
    call('ptv_scatter_rows', ptr(dns), ptr(dns_s), ptr(perm), R, Ht, 0, 0, 1, stream_ptr())


tok_old(); tok(dtok_m, perm); ns_old(); ns(dns_m, perm); torch.cuda.synchronize()
assert torch.equal(dtok, dtok_m) and torch.equal(dns, dns_m)
for name, f in (('dtok: product (sorted order) + ptv_scatter_rows_seg', tok_old), ('dtok: product alone (sorted order)', lambda: tok(dtok_s, None)),
                ('dtok: product storing through perm', lambda: tok(dtok_m, perm)),
                ('dNS: two products (sorted order) + ptv_scatter_rows', ns_old), ('dNS: two products alone (sorted order)', lambda: ns(dns_s, None)),
                ('dNS: two products storing through perm', lambda: ns(dns_m, perm))):
    print('%-64s %8.1f us' % (name, best_us(f)))
