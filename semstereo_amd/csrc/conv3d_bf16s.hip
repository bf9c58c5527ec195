// The tiled split-operand conv kernel's own translation unit: the packing of its weights and the entry points of the plain 3-D
// (stride 1 and 2) and 2-D forms.  The kernel template, its header comment and the launch helpers are in conv3d_bf16s.h.
#include "conv3d_bf16s.h"

namespace {

// [Cout,Cin,3,3,3] fp32 -> [ceil(Cin/8)][14 steps][3 terms][2 halves][Cout][8] bf16 (zero padded)
__global__ void pack_weights_bf16s_kernel(const float* __restrict__ w, unsigned short* __restrict__ wsplit, int Cout,
                                          int Cin, int ktaps, long long total) {
    const int KSTEPS = (ktaps + 1) / 2;                        // 14 (3x3x3) or 5 (3x3)
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int j = (int)(i % 8);
    long long r = i / 8;
    const int co = (int)(r % Cout); r /= Cout;
    const int half = (int)(r % 2); r /= 2;
    const int term = (int)(r % 3); r /= 3;
    const int s = (int)(r % KSTEPS);
    const int blk = (int)(r / KSTEPS);
    const int tap = 2 * s + half, ci = blk * 8 + j;
    float x = 0.f;
    if (tap < ktaps && ci < Cin) x = w[((long long)co * Cin + ci) * ktaps + tap];
    unsigned h, m, l;
    split3(x, h, m, l);
    wsplit[i] = (unsigned short)(term == 0 ? h : (term == 1 ? m : l));
}

// f16 form: per output channel, the power of two that brings max |w| into [2^14, 2^15) -- its inverse is stored behind the packed terms
// (float[Cout]) for the conv kernel's epilogue -- then [Cout,Cin,taps] fp32 -> [ceil(Cin/8)][steps][2 terms][2 halves][Cout][8] fp16 of
// w / wunscale[co].  One workgroup per output channel does both (r06: they were two launches, and training re-packs every layer's
// weights every step: ~100 small launches per step; same arithmetic on the same values, bit-identical output).
__global__ __launch_bounds__(256) void pack_weights_f16s_fused_kernel(const float* __restrict__ w, unsigned short* __restrict__ wsplit,
                                                                       float* __restrict__ wunscale, int Cout, int Cin, int ktaps) {
    __shared__ unsigned wmax[4];
    const int co = blockIdx.x, per_co = Cin * ktaps;
    const float* wc = w + (size_t)co * per_co;
    float m = 0.f;
    for (int i = threadIdx.x; i < per_co; i += 256) m = fmaxf(m, fabsf(wc[i]));
    const float u = weight_unscale(m, wmax);
    if (threadIdx.x == 0) wunscale[co] = u;
    const int KSTEPS = (ktaps + 1) / 2, nblk = (Cin + 7) / 8;
    const int n = nblk * KSTEPS * 4 * 8;                      // this channel's slots: (blk, s, term, half, j)
    for (int e = threadIdx.x; e < n; e += 256) {
        const int j = e % 8;
        int r = e / 8;
        const int half = r % 2; r /= 2;
        const int term = r % 2; r /= 2;
        const int s = r % KSTEPS;
        const int blk = r / KSTEPS;
        const int tap = 2 * s + half, ci = blk * 8 + j;
        float x = 0.f;
        if (tap < ktaps && ci < Cin) x = wc[(size_t)ci * ktaps + tap] / u;       // exact: a power of two
        const long long i = ((((long long)(blk * KSTEPS + s) * 2 + term) * 2 + half) * Cout + co) * 8 + j;
        wsplit[i] = split_weight_f16(x, term);
    }
}

}  // namespace

static int check_conv_args(const ConvArgs& a, int nterms) {      // (2-D: D = 1)
    SS_REQUIRE(a.in && a.wsplit && a.out && a.B > 0 && a.Cin > 0 && a.D > 0 && a.H > 0 && a.W > 0 && a.Cout > 0);
    SS_REQUIRE((nterms == 3 || nterms == 6 || nterms == F16X3) && (reinterpret_cast<uintptr_t>(a.wsplit) & 15) == 0);
    // operands are addressed through 32-bit buffer offsets: one batch element's input must stay below 2 GiB
    return (long long)a.Cin * a.D * a.H * a.W * 4 >= 0x7fffffffLL ? SS_ERR_UNSUPPORTED : SS_OK;
}

static int conv3d_bf16s_impl(const ConvArgs& a, int stride, int nterms) {
    SS_REQUIRE(stride == 1 || stride == 2);
    if (const int rc = check_conv_args(a, nterms); rc != SS_OK) return rc;
    const int Do = (a.D - 1) / stride + 1, Ho = (a.H - 1) / stride + 1, Wo = (a.W - 1) / stride + 1;
    if ((long long)a.Cout * Do * Ho * Wo * 4 >= 0x7fffffffLL) return SS_ERR_UNSUPPORTED;      // ... and so must its output
    const ss::ConvPlan plan = ss::plan_conv3d(Do, Ho, Wo, a.Cout, a.B, stride, nterms, a.gate != nullptr, ss::fill_hint(),
                                              ss::tuning().conv_tile, ss::tuning().conv_s2_mt1);
    return ss::with_int<3, 6, F16X3>(nterms, [&](auto nt) {
        auto launch = [&](auto tile) {
            return with_gate_and_accb(tile, a.gate != nullptr, plan.accb, [&](auto form) {
                using F = decltype(form);
                if constexpr (F::S == 2 && !F::GATED) {
                    if (plan.s2 == ss::S2Form::split_channels) return launch_conv(form.split_channels(), a);
                }
                if constexpr (F::S == 2) {
                    if (plan.s2 == ss::S2Form::two_channel_tiles) return launch_conv(form.two_channel_tiles(), a);
                }
                return launch_conv(form, a);
            });
        };
        // stride 2 needs a 65-column halo tile per row.  A 1 x 4 output tile is 84 KB of split operands: one workgroup per
        // CU, slower than the exact-fp32 kernel (283 vs 229 us on the largest layer).  A 2 x 2 tile is 78 KB (5 x 5 x 65 halo positions): two
        // workgroups per CU, faster on every stride-2 layer of the model (190 / 95 / 68 / 41 us vs 229 / 122 / 81 / 62).
        if (stride == 2) return launch(ConvForm<2, 1, 2, 2, decltype(nt)::value>{});
        return with_stride1_tile<decltype(nt)::value>(plan.tile, launch);
    });
}

extern "C" int ss_conv3d_bf16s_fwd(const float* in, const void* wsplit, const float* scale, const float* shift,
                                   const float* residual, const float* gate, float* out, int B, int Cin, int D, int H,
                                   int W, int Cout, int stride, int relu, int nterms, ss_stream_t stream) {
    ConvArgs a;
    a.in = in; a.wsplit = wsplit; a.scale = scale; a.shift = shift; a.residual = residual; a.gate = gate; a.out = out;
    a.B = B; a.Cin = Cin; a.D = D; a.H = H; a.W = W; a.Cout = Cout; a.relu = relu != 0; a.stream = ss::as_stream(stream);
    return conv3d_bf16s_impl(a, stride, nterms);
}

extern "C" int ss_conv3d_bf16s_partial_fwd(const float* in, const void* wsplit, const float* partial, const float* scale,
                                           const float* shift, const float* gate, float* out, int B, int Cin, int D,
                                           int H, int W, int Cout, int relu, int nterms, ss_stream_t stream) {
    SS_REQUIRE(partial != nullptr);
    ConvArgs a;
    a.in = in; a.wsplit = wsplit; a.scale = scale; a.shift = shift; a.residual = partial; a.residual_is_partial_sum = true; a.gate = gate; a.out = out;
    a.B = B; a.Cin = Cin; a.D = D; a.H = H; a.W = W; a.Cout = Cout; a.relu = relu != 0; a.stream = ss::as_stream(stream);
    return conv3d_bf16s_impl(a, 1, nterms);
}

extern "C" int ss_conv3d_bf16s_cl_fwd(const float* in, const void* wsplit, const float* scale, const float* shift, float* out,
                                      int B, int Cin, int D, int H, int W, int Cout, int relu, int nterms, ss_stream_t stream) {
    SS_REQUIRE(Cout > 0 && Cout % 8 == 0);
    ConvArgs a;
    a.in = in; a.wsplit = wsplit; a.scale = scale; a.shift = shift; a.out = out; a.channels_last = true;
    a.B = B; a.Cin = Cin; a.D = D; a.H = H; a.W = W; a.Cout = Cout; a.relu = relu != 0; a.stream = ss::as_stream(stream);
    return conv3d_bf16s_impl(a, 1, nterms);
}

// The packed weights of the 3x3x3 (ktaps 27) and 3x3 (ktaps 9) convs, the one statement of their size:
// [ceil(Cin/8)][ceil(ktaps/2) tap pairs][3 bf16 or 2 fp16 terms][2 halves][Cout][8] two-byte terms, then (fp16 form) float[Cout].
static ss::Packed conv_packed(int Cout, int Cin, int ktaps, bool f16) {
    const long long terms = (long long)ss::ceil_div(Cin, 8) * ((ktaps + 1) / 2) * (f16 ? 2 : 3) * 2 * Cout * 16;
    return {terms, terms + (f16 ? 4LL * Cout : 0)};
}

static int conv_packed_bytes(int Cout, int Cin, int ktaps, bool f16, long long* bytes) {
    SS_REQUIRE(bytes && Cout > 0 && Cin > 0);
    *bytes = conv_packed(Cout, Cin, ktaps, f16).total;
    return SS_OK;
}

static int pack_conv_bf16s(const float* w, void* wsplit, int Cout, int Cin, int ktaps, ss_stream_t stream) {
    SS_REQUIRE(w && wsplit && Cout > 0 && Cin > 0);
    const long long total = conv_packed(Cout, Cin, ktaps, false).terms / 2;
    hipLaunchKernelGGL(pack_weights_bf16s_kernel, dim3((unsigned)ss::ceil_div_ll(total, 256)), dim3(256), 0,
                       ss::as_stream(stream), w, reinterpret_cast<unsigned short*>(wsplit), Cout, Cin, ktaps, total);
    return ss::check_launch();
}

// the two-term fp16 form of the same weights (nterms = 19 of ss_conv3d_bf16s_fwd): see the top of conv3d_bf16s.h
static int pack_conv_f16s(const float* w, void* wsplit, int Cout, int Cin, int ktaps, ss_stream_t stream) {
    SS_REQUIRE(w && wsplit && Cout > 0 && Cin > 0);
    hipLaunchKernelGGL(pack_weights_f16s_fused_kernel, dim3(Cout), dim3(256), 0, ss::as_stream(stream), w, reinterpret_cast<unsigned short*>(wsplit),
                       ss::scales_of(wsplit, conv_packed(Cout, Cin, ktaps, true)), Cout, Cin, ktaps);
    return ss::check_launch();
}

extern "C" int ss_pack_conv3d_weights_bf16s(const float* w, void* wsplit, int Cout, int Cin, ss_stream_t stream) {
    return pack_conv_bf16s(w, wsplit, Cout, Cin, 27, stream);
}
extern "C" int ss_pack_conv3d_weights_bf16s_bytes(int Cout, int Cin, long long* bytes) { return conv_packed_bytes(Cout, Cin, 27, false, bytes); }
extern "C" int ss_pack_conv3d_weights_f16s(const float* w, void* wsplit, int Cout, int Cin, ss_stream_t stream) {
    return pack_conv_f16s(w, wsplit, Cout, Cin, 27, stream);
}
extern "C" int ss_pack_conv3d_weights_f16s_bytes(int Cout, int Cin, long long* bytes) { return conv_packed_bytes(Cout, Cin, 27, true, bytes); }

// ---- the 2-D form: Conv2d(k3, s1, p1, bias=False) + affine + optional residual + ReLU on [B,C,H,W] maps (concat_feature of
// the reference model, models/SemStereo.py:222-226): the same kernel with a depth-1 volume and 9 taps (5 K-steps) ----
extern "C" int ss_pack_conv2d_weights_bf16s(const float* w, void* wsplit, int Cout, int Cin, ss_stream_t stream) {
    return pack_conv_bf16s(w, wsplit, Cout, Cin, 9, stream);
}
extern "C" int ss_pack_conv2d_weights_bf16s_bytes(int Cout, int Cin, long long* bytes) { return conv_packed_bytes(Cout, Cin, 9, false, bytes); }
extern "C" int ss_pack_conv2d_weights_f16s(const float* w, void* wsplit, int Cout, int Cin, ss_stream_t stream) {
    return pack_conv_f16s(w, wsplit, Cout, Cin, 9, stream);
}
extern "C" int ss_pack_conv2d_weights_f16s_bytes(int Cout, int Cin, long long* bytes) { return conv_packed_bytes(Cout, Cin, 9, true, bytes); }

// (the plain and the concat-free form -- a.rem set -- get the same tile for the same launch: the two are bit-identical)
static int conv2d_bf16s_impl(const ConvArgs& a, int nterms) {
    if (const int rc = check_conv_args(a, nterms); rc != SS_OK) return rc;
    const int rows = ss::plan_conv2d_rows(a.H, a.W, a.Cout, a.B);
    return ss::with_int<3, 6, F16X3>(nterms, [&](auto nt) {
        constexpr int NTERMS = decltype(nt)::value;
        auto launch = [&](auto tile) {
            const auto form = tile.conv2d().accb(ss::bool_c<NTERMS == F16X3 && ss::kConv2dAccb>{});
            return ss::with_bool(a.rem != nullptr, [&](auto cat) { return launch_conv(form.cat(cat), a); });
        };
        if (rows == 16) return launch(ConvForm<1, 4, 1, 16, NTERMS>{});
        if (rows == 8) return launch(ConvForm<1, 2, 1, 8, NTERMS>{});
        return launch(ConvForm<1, 1, 1, 4, NTERMS>{});
    });
}

extern "C" int ss_conv2d_bf16s_fwd(const float* in, const void* wsplit, const float* scale, const float* shift,
                                   const float* residual, float* out, int B, int Cin, int H, int W, int Cout, int relu,
                                   int nterms, ss_stream_t stream) {
    ConvArgs a;
    a.in = in; a.wsplit = wsplit; a.scale = scale; a.shift = shift; a.residual = residual; a.out = out;
    a.B = B; a.Cin = Cin; a.H = H; a.W = W; a.Cout = Cout; a.relu = relu != 0; a.stream = ss::as_stream(stream);
    return conv2d_bf16s_impl(a, nterms);
}

extern "C" int ss_conv2d_bf16s_pair_fwd(const float* in_a, const float* in_b, const void* wsplit, const float* scale,
                                        const float* shift, float* out, int B, int Cin, int H, int W, int Cout, int relu,
                                        int nterms, ss_stream_t stream) {
    SS_REQUIRE(in_a && in_b);
    ConvArgs a;
    a.in = in_a; a.in_second_view = in_b; a.bsplit = B; a.wsplit = wsplit; a.scale = scale; a.shift = shift; a.out = out;
    a.B = 2 * B; a.Cin = Cin; a.H = H; a.W = W; a.Cout = Cout; a.relu = relu != 0; a.stream = ss::as_stream(stream);
    return conv2d_bf16s_impl(a, nterms);
}

// The concat-free form (CAT of the kernel): channels [0, Csplit) of the convolution's input from x_a, [Csplit, Cin) from rem_a; with
// x_b / rem_b the launch serves two views (out [2B,Cout,H,W]: elements 0..B-1 from the _a pair, B..2B-1 from the _b pair).
extern "C" int ss_conv2d_bf16s_cat_fwd(const float* x_a, const float* rem_a, const float* x_b, const float* rem_b, const void* wsplit,
                                       const float* scale, const float* shift, float* out, int B, int Csplit, int Cin, int H, int W,
                                       int Cout, int relu, int nterms, ss_stream_t stream) {
    SS_REQUIRE(x_a && rem_a && (x_b == nullptr) == (rem_b == nullptr));
    SS_REQUIRE(B > 0 && Csplit > 0 && Csplit < Cin);
    if (Csplit % 8 != 0) return SS_ERR_UNSUPPORTED;            // a staged 8-channel chunk would straddle the two tensors
    const bool pair = x_b != nullptr;
    ConvArgs a;
    a.in = x_a; a.in_second_view = x_b; a.rem = rem_a; a.rem_second_view = rem_b; a.bsplit = pair ? B : 0; a.csplit = Csplit;
    a.wsplit = wsplit; a.scale = scale; a.shift = shift; a.out = out;
    a.B = pair ? 2 * B : B; a.Cin = Cin; a.H = H; a.W = W; a.Cout = Cout; a.relu = relu != 0; a.stream = ss::as_stream(stream);
    return conv2d_bf16s_impl(a, nterms);
}
