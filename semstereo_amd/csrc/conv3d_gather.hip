// concat_stem with the sparse concat volume formed INSIDE its staging (second half; reference
// models/SemStereo.py:241-244, 316-320, models/submodule.py:265-288): the GATHER form of conv3d_bf16s, instantiated in its own
// translation unit so that the two files compile side by side.  See the kernel's header comment in conv3d_bf16s.h.
#include "conv3d_bf16s.h"

extern "C" int ss_conv3d_gather_fwd(const float* right, const float* cand, const float* att, const void* wsplit,
                                    const float* partial, const float* scale, const float* shift, const float* gate, float* out,
                                    int B, int Cin, int nd, int H, int W, int Cout, int relu, int nterms, ss_stream_t stream) {
    SS_REQUIRE(right && cand && att && wsplit && out);
    SS_REQUIRE(B > 0 && Cin >= 16 && Cin % 8 == 0 && nd > 0 && H > 0 && W > 0 && Cout > 0);
    SS_REQUIRE((reinterpret_cast<uintptr_t>(wsplit) & 15) == 0);
    if (nterms != F16X3) return SS_ERR_UNSUPPORTED;             // the two-term fp16 engine (the default) only
    if ((long long)Cin * H * W * 4 >= 0x7fffffffLL || (long long)nd * H * W * 4 >= 0x7fffffffLL) return SS_ERR_UNSUPPORTED;
    if ((long long)Cout * nd * H * W * 4 >= 0x7fffffffLL) return SS_ERR_UNSUPPORTED;
    ConvArgs a;
    a.in = right; a.candidates = cand; a.attention = att; a.wsplit = wsplit; a.residual = partial; a.residual_is_partial_sum = partial != nullptr;
    a.scale = scale; a.shift = shift; a.gate = gate; a.out = out;
    a.B = B; a.Cin = Cin; a.D = nd; a.H = H; a.W = W; a.Cout = Cout; a.relu = relu != 0; a.stream = ss::as_stream(stream);
    // tile choice and chunk-blocked accumulation: the plan of a stride-1 layer of this output shape
    const ss::ConvPlan plan = ss::plan_conv3d(nd, H, W, Cout, B, 1, nterms, gate != nullptr, ss::fill_hint(), ss::tuning().conv_tile,
                                              ss::tuning().conv_s2_mt1);
    return with_stride1_tile<F16X3>(plan.tile, [&](auto tile) {
        return with_gate_and_accb(tile, gate != nullptr, plan.accb, [&](auto form) { return launch_conv(form.gather(), a); });
    });
}
