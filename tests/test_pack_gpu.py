"""GPU: what each `ss_pack_*` kernel WRITES against what `ss_pack_*_bytes` says the buffer holds.  The raw entry point fills a buffer
of the queried size plus a guard, twice, over two different sentinels: the guard must survive, the two results must agree wherever
something was written, the written extent must end inside the last 16 bytes of the queried size, and the Python wrapper must return
exactly that buffer."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096                                                    # bytes behind the queried size
SENTINELS = (0x5A5A, -0x2B2C)


def _w(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).cuda()


def _engine():
    import semstereo_amd
    return semstereo_amd.engine


def _k4s2(w):
    from semstereo_amd import train_decoder
    return train_decoder.pack_conv2d_k4s2_weight(w)


def _stem(w):
    from semstereo_amd import ops
    return ops.pack_stem_left_weights_f16s(w)


#: entry point -> (its scalar arguments -> the weight's shape, the Python wrapper, the argument tuples it is packed at).  The
#: dimensions are the smallest at which a layout can go wrong: a channel count below one tile (32), one that is no multiple of it, an
#: input-channel count that is no multiple of the chunk (8, 16 or 32) where the pack takes one.
PACKS = {
    "ss_pack_conv3d_weights_bf16s": (lambda Cout, Cin: (Cout, Cin, 3, 3, 3), lambda w: _engine().pack_conv_weight_bf16s(w, 6),
                                     ((6, 8), (33, 17), (40, 70))),
    "ss_pack_conv3d_weights_f16s": (lambda Cout, Cin: (Cout, Cin, 3, 3, 3), lambda w: _engine().pack_conv_weight_bf16s(w, 19),
                                    ((6, 8), (33, 17), (40, 70))),
    "ss_pack_conv2d_weights_bf16s": (lambda Cout, Cin: (Cout, Cin, 3, 3), lambda w: _engine().pack_conv2d_weight_bf16s(w, 6),
                                     ((6, 8), (33, 17), (40, 70))),
    "ss_pack_conv2d_weights_f16s": (lambda Cout, Cin: (Cout, Cin, 3, 3), lambda w: _engine().pack_conv2d_weight_bf16s(w, 19),
                                    ((6, 8), (33, 17), (40, 70))),
    "ss_pack_deconv3d_weights_bf16s": (lambda Cin, Cout, ntaps: (Cin, 27, Cout) if ntaps == 27 else (Cin, Cout),
                                       lambda w: _engine().pack_deconv_weight_bf16s(w, 6), ((8, 6, 27), (17, 33, 27), (70, 40, 1))),
    "ss_pack_deconv3d_weights_f16s": (lambda Cin, Cout: (Cin, 27, Cout), lambda w: _engine().pack_deconv_weight_bf16s(w, 19),
                                      ((8, 6), (17, 33), (70, 40))),
    "ss_pack_deconv2d_weights_f16s": (lambda Cin, Cout: (Cin, Cout, 4, 4), lambda w: _engine().pack_deconv2d_weight(w),
                                      ((8, 6), (17, 33), (70, 40))),
    "ss_pack_conv2d_k4s2_weights_f16s": (lambda Cout, Cin: (Cout, Cin, 4, 4), _k4s2, ((6, 8), (33, 17), (40, 70))),
    "ss_pack_conv2d_k1_weights_f16s": (lambda Cout, Cin: (Cout, Cin, 1, 1), lambda w: _engine().pack_conv2d_k1_weight(w),
                                       ((6, 8), (33, 17), (40, 70))),
    "ss_pack_seghead_weights_f16s": (lambda Cin: (32, Cin, 3, 3), lambda w: _engine().pack_seghead_weight(w), ((8,), (24,))),
    "ss_pack_conv3d_head_weights_bf16s": (lambda Cin: (1, Cin, 3, 3, 3), lambda w: _engine().pack_head_weight_bf16s(w, 6), ((16,), (64,))),
    "ss_pack_conv3d_head_weights_f16s": (lambda Cin: (1, Cin, 3, 3, 3), lambda w: _engine().pack_head_weight_bf16s(w, 19), ((16,), (64,))),
    "ss_pack_pointwise_weights_bf16s": (lambda Cout, Cin: (Cout, Cin), lambda w: _engine().pack_pointwise_weight_bf16s(w),
                                        ((33, 16), (40, 48))),
    "ss_pack_stem_left_weights_f16s": (lambda Cout, C: (Cout, C, 27), _stem, ((32, 32),)),
    "ss_pack_classifier_head_weights": (lambda: (1, 32, 3, 3, 3), lambda w: _engine().pack_classifier_head_weight(w), ((),)),
}


def raw_pack(name, w, dims, sentinel=0, guard=0):
    """The raw entry point into queried bytes + `guard` bytes of `sentinel` -> (the int16 buffer, the queried bytes)."""
    from semstereo_amd import _lib
    n = _lib.query_bytes(name + "_bytes", *dims)
    assert n > 0 and n % 2 == 0 and guard % 2 == 0
    buf = torch.full(((n + guard) // 2,), sentinel, dtype=torch.int16, device=w.device)
    with torch.cuda.device(w.device):
        _lib.call(name, _lib.ptr(w), _lib.ptr(buf), *dims)
    torch.cuda.synchronize()
    return buf, n


@pytest.mark.parametrize("name", sorted(PACKS))
def test_the_pack_writes_what_the_query_says(name):
    shape, wrapper, cases = PACKS[name]
    for k, dims in enumerate(cases):
        w = _w(shape(*dims), 1000 + k)
        runs = []
        for s in SENTINELS:
            buf, n = raw_pack(name, w, dims, s, GUARD)
            assert buf.numel() * 2 == n + GUARD
            assert bool((buf[n // 2:] == s).all()), (name, dims, "the guard behind the queried size was written")
            runs.append(buf[:n // 2].clone())
        written = ~((runs[0] == SENTINELS[0]) & (runs[1] == SENTINELS[1]))
        assert torch.equal(runs[0][written], runs[1][written]), (name, dims)
        e = 2 * (int(written.nonzero().max()) + 1)              # the written extent in bytes
        print(f"{name}{dims}: queried {n} bytes, written extent {e}, {int((~written).sum())} elements unwritten")
        assert e <= n <= (e + 15) // 16 * 16, (name, dims, e, n)
        # every layout zero-pads, so all of [0, e) is written; only the head's fp16 form has a tail (one float in 16 bytes)
        assert bool(written[:e // 2].all()) and (e == n or name == "ss_pack_conv3d_head_weights_f16s"), (name, dims, e, n)
        out = wrapper(w)
        assert out.dtype == torch.int16 and out.numel() * 2 == n, (name, dims, out.numel())
        assert torch.equal(out[written], runs[0][written]), (name, dims)
