// Weight gradient of Conv2d(C0 + C1, Cout, 3, stride 1, padding 1, bias=False) applied to cat((in0, in1), 1), the concatenation never
// formed -- conv2 of every 2-D Conv2x (models/submodule.py:142, 157-160), `concat_feature` (models/SemStereo.py:221-223) and the 3x3
// conv1 of `segmenthead` (the class whose forward is models/submodule.py:40-52) -- for training the 2-D decoder and the heads:
//
//   gw[co, ci, kh, kw] = sum_{b,y,x} g[b, co, y, x] * in[b, ci, y + kh - 1, x + kw - 1]        (zero padding; ci < C0: in0, else in1)
//
// (ss_conv2d_k3_wgrad_fwd.)  Until now these layers took the 3x3x3 kernel on depth-1 volumes (conv3d_wgrad_bf16s.hip), 18 of whose 27
// taps multiply padding planes, once per source, with fp32 atomics.  Here: a GEMM with M = 32 output channels (g, lane = co), N = 32
// input channels (lane = ci) per tap, K = positions, on the three-term bf16 form (split_bf16.h, six products, smallest first, on
// v_mfma_f32_32x32x16_bf16, fp32 accumulators) in the arithmetic and order of ss_deconv2d_k4s2_wgrad_fwd.
//
// A workgroup = one (co tile, ci tile) and a range of rows (b, y); its three waves are the three kh, each with its three kw (48
// accumulator registers).  A 32-channel input tile belongs to ONE source (tiles number ceil(C0/32) + ceil(C1/32) along ci), so the
// source boundary never falls inside a tile and no lane chooses a pointer.  The workgroup walks down 32-column chunks of its rows.  Per
// step (row y, chunk w0) the 192 threads stage, with row-major loads (16 lanes = one channel's 128-byte run) split ONCE at staging time:
//   * the g chunk [32 co][32 positions] into one of two buffers ([term][co] rows of 64 bytes, stride 80), shared by the three waves;
//   * input row y + 1 [32 ci][32 + 2 halo] into a ring of four row tiles ([term][ci] rows [8 pad | 32 | 8 pad] bf16, stride 112): input
//     row r serves kh = 0, 1, 2 of output rows r + 1, r, r - 1, so each row is staged once per workgroup and chunk, not three times
//     (the two rows above a range's first are staged when the walk starts).
// Everything outside the maps -- left / right padding, ragged W, channels beyond C0 / C1 / Cout -- is a zero at staging time.  The three
// kw taps are the staged row read at offsets -1, 0, +1: kw = 1 the aligned 16-byte word, kw = 0 / 2 that word shifted by one element
// (v_alignbit with one neighbouring dword), as in conv3d_wgrad_bf16s.hip.  Row strides of 112 / 80 bytes = 28 / 20 dwords: the sixteen
// lanes that a 16-byte LDS read serves per cycle have sixteen different l mod 16, and 7 l mod 16 / 5 l mod 16 are permutations, so the
// fragment reads are conflict-free; the two neighbouring-dword reads per term are 4-way conflicts (28 l mod 32 takes 8 values).
// A kh whose input row lies in the padding is skipped wave-uniformly.  One barrier per step: at step y the workgroup writes row y + 1
// into ring slot (y + 2) & 3 and g row y into buffer y & 1 (both loaded a step ago), meets, issues the loads of step y + 1 and
// multiplies -- a wave still multiplying step y - 1 reads the slots of rows y - 2, y - 1, y and buffer (y - 1) & 1, none being written.
//
// Each workgroup writes ONE partial [9 taps][32 co][32 ci] block (36 864 bytes) into the workspace; a second, small launch adds a
// tile's partials in a fixed order in double and rounds once.  No floating-point atomics: the same inputs give the same bits.  The
// partition of the rows into partials is a function of the geometry alone (k3_plan, the rule of deconv2d_train.hip's wgrad_plan).
#include "common.h"
#include "split_bf16.h"

namespace {

constexpr int CW = 32;                                     // positions per chunk: two K-steps of 16
constexpr int IRS = 112, IPLANE = 32 * IRS, ITILE = 3 * IPLANE;      // one input row tile: [term][ci][8 pad | 32 | 8 pad] bf16
constexpr int ARS = 80, APLANE = 32 * ARS, ATILE = 3 * APLANE;       // one g chunk: [term][co][32] bf16
constexpr int RING = 4;
constexpr int LDS_BYTES = RING * ITILE + 2 * ATILE;       // 58 368
constexpr int PART = 9 * 1024;                             // floats per partial block

struct K3Plan {
    int rpp, nparts, nci0, nci, nco;
};
// rows per partial and partials per weight tile: a partial covers at least 2048 positions, at most clamp(1024 / tiles, 1, 256) of them
inline K3Plan k3_plan(int B, int C0, int C1, int H, int W, int Cout) {
    K3Plan p;
    p.nci0 = ss::ceil_div(C0, 32);
    p.nci = p.nci0 + ss::ceil_div(C1, 32);
    p.nco = ss::ceil_div(Cout, 32);
    const long long rows = (long long)B * H, tiles = (long long)p.nci * p.nco;
    long long cap = 1024 / tiles;
    cap = cap < 1 ? 1 : (cap > 256 ? 256 : cap);
    long long rpp = ss::ceil_div_ll(rows, cap);
    const long long floor_rows = ss::ceil_div_ll(2048, W);
    if (rpp < floor_rows) rpp = floor_rows;
    if (rpp > rows) rpp = rows;
    p.rpp = (int)rpp;
    p.nparts = (int)ss::ceil_div_ll(rows, rpp);
    return p;
}

// grid (nparts, nco * nci); wave = kh
__global__ __launch_bounds__(192) void conv2d_k3_wgrad_bf16s(const float* __restrict__ g, const float* __restrict__ in0,
                                                             const float* __restrict__ in1, float* __restrict__ ws, int C0, int C1, int H,
                                                             int W, int Cout, long long rows, int rpp, int nci0, int nci) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    unsigned char* const abuf = lds + RING * ITILE;
    const int tid = threadIdx.x, lane = tid & 63, kh = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int part = blockIdx.x, tile = blockIdx.y;
    const int tco = tile / nci, tci = tile - tco * nci;
    const int co0 = tco * 32;
    // the source of this input tile (workgroup-uniform)
    const bool second = tci >= nci0;
    const float* __restrict__ src = second ? in1 : in0;
    const int Cs = second ? C1 : C0, ci0 = (second ? tci - nci0 : tci) * 32;
    const size_t plane = (size_t)H * W;

    // staging: pair p = tid + 192 k (k < 3, p < 512): channel p >> 4, positions 2 (p & 15) and + 1; halo: threads 0-63.  Buffer loads
    // with the masks folded into the per-lane offset (0x80000000 is beyond any element: the load returns 0) -- no vector-memory
    // instruction stands under a branch, so the loads of step y + 1 stay in flight under the MFMAs of step y.  The offsets depend on
    // the chunk alone (chunk_offsets), the row is the scalar offset.
    constexpr unsigned OOB = 0x80000000u;
    const int hch = tid & 31, hside = (tid >> 5) & 1;
    unsigned vg[3][2], vi[3][2], vh = OOB;
    auto chunk_offsets = [&](int w0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int p = tid + 192 * k, ch = p >> 4, x = w0 + 2 * (p & 15);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const bool okx = p < 512 && x + e < W;
                vg[k][e] = (okx && co0 + ch < Cout) ? (unsigned)(((size_t)(co0 + ch) * plane + x + e) * 4) : OOB;
                vi[k][e] = (okx && ci0 + ch < Cs) ? (unsigned)(((size_t)(ci0 + ch) * plane + x + e) * 4) : OOB;
            }
        }
        const int x = hside ? w0 + CW : w0 - 1;
        vh = (tid < 64 && ci0 + hch < Cs && (unsigned)x < (unsigned)W) ? (unsigned)(((size_t)(ci0 + hch) * plane + x) * 4) : OOB;
    };
    __amdgpu_buffer_rsrc_t gres, ires;
    auto element = [&](int b) {                             // (one element's tensors stay below 2 GiB: k3_check)
        gres = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g + (size_t)b * Cout * plane), 0, (int)((size_t)Cout * plane * 4), 0x00020000);
        ires = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(src + (size_t)b * Cs * plane), 0, (int)((size_t)Cs * plane * 4), 0x00020000);
    };
    float rg[3][2], ri[3][2], rh = 0.f;
    auto load_g = [&](int y) {
        const int row_b = y * W * 4;
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int e = 0; e < 2; ++e) rg[k][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(gres, (int)vg[k][e], row_b, 0));
    };
    bool rok = false;                                       // (scalar) the row in `ri` / `rh` lies inside the map
    auto load_i = [&](int r) {                              // a row in the padding: zeros at store time (and no wave reads it)
        rok = (unsigned)r < (unsigned)H;
        const int row_b = rok ? r * W * 4 : 0;
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int e = 0; e < 2; ++e) ri[k][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ires, (int)vi[k][e], row_b, 0));
        rh = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ires, (int)vh, row_b, 0));
    };
    auto store_g = [&](int buf) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int p = tid + 192 * k;
            if (p < 512) {
                unsigned h, m, l;
                split3_pk(rg[k][0], rg[k][1], h, m, l);
                unsigned char* q = abuf + buf * ATILE + (p >> 4) * ARS + 4 * (p & 15);
                *reinterpret_cast<unsigned*>(q) = h;
                *reinterpret_cast<unsigned*>(q + APLANE) = m;
                *reinterpret_cast<unsigned*>(q + 2 * APLANE) = l;
            }
        }
    };
    auto store_i = [&](int slot) {
        unsigned char* t = lds + slot * ITILE;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int p = tid + 192 * k;
            if (p < 512) {
                unsigned h, m, l;
                split3_pk(rok ? ri[k][0] : 0.f, rok ? ri[k][1] : 0.f, h, m, l);
                unsigned char* q = t + (p >> 4) * IRS + 16 + 4 * (p & 15);
                *reinterpret_cast<unsigned*>(q) = h;
                *reinterpret_cast<unsigned*>(q + IPLANE) = m;
                *reinterpret_cast<unsigned*>(q + 2 * IPLANE) = l;
            }
        }
        if (tid < 64) {                                    // the halo elements of channel hch: element 7 (left) / 40 (right) of the row
            unsigned h, m, l;
            split3_pk(rok ? rh : 0.f, 0.f, h, m, l);
            unsigned char* q = t + hch * IRS + (hside ? 80 : 14);
            *reinterpret_cast<unsigned short*>(q) = (unsigned short)h;
            *reinterpret_cast<unsigned short*>(q + IPLANE) = (unsigned short)m;
            *reinterpret_cast<unsigned short*>(q + 2 * IPLANE) = (unsigned short)l;
        }
    };

    f32x16 acc[3];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const long long r0 = (long long)part * rpp, r1 = (r0 + rpp < rows) ? r0 + rpp : rows;
    long long row = r0;
    while (row < r1) {
        // a segment: the rows ya .. yb - 1 of batch element b
        const int b = (int)(row / H), ya = (int)(row - (long long)b * H);
        const int yb = (r1 - row < (long long)(H - ya)) ? ya + (int)(r1 - row) : H;
        element(b);
        for (int w0 = 0; w0 < W; w0 += CW) {
            chunk_offsets(w0);
            __syncthreads();                               // every wave has left the previous walk's tiles
            load_i(ya - 1);
            store_i(ya & 3);                               // (input row r lives in slot (r + 1) & 3)
            load_i(ya);
            store_i((ya + 1) & 3);
            load_g(ya);
            load_i(ya + 1);
            for (int y = ya; y < yb; ++y) {
                store_g(y & 1);
                store_i((y + 2) & 3);
                __syncthreads();
                // the next step's loads fly under this step's MFMAs (unconditional: the last step loads its own rows again)
                const int yn = y + 1 < yb ? y + 1 : y;
                load_g(yn);
                load_i(yn + 1);
                const int r = y + kh - 1;
                if ((unsigned)r >= (unsigned)H) continue;  // (wave-uniform: this kh's input row lies in the padding)
                const unsigned char* at = abuf + (y & 1) * ATILE + l31 * ARS + 16 * half;
                const unsigned char* bt = lds + ((r + 1) & 3) * ITILE + l31 * IRS + 16 * (1 + half);
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if (w0 + 16 * s >= W) break;           // (uniform: a K-step beyond the row is all zeros)
                    uint4 af[3], bfr[3][3];                // [term], [kw][term]
#pragma unroll
                    for (int t = 0; t < 3; ++t) {
                        af[t] = *reinterpret_cast<const uint4*>(at + t * APLANE + 32 * s);
                        const unsigned char* bp = bt + t * IPLANE + 32 * s;
                        const uint4 x = *reinterpret_cast<const uint4*>(bp);
                        const unsigned pl = *reinterpret_cast<const unsigned*>(bp - 4), nf = *reinterpret_cast<const unsigned*>(bp + 16);
                        const unsigned a0 = __builtin_amdgcn_alignbit(x.x, pl, 16), a1 = __builtin_amdgcn_alignbit(x.y, x.x, 16);
                        const unsigned a2 = __builtin_amdgcn_alignbit(x.z, x.y, 16), a3 = __builtin_amdgcn_alignbit(x.w, x.z, 16);
                        const unsigned a4 = __builtin_amdgcn_alignbit(nf, x.w, 16);
                        bfr[0][t] = make_uint4(a0, a1, a2, a3);
                        bfr[1][t] = x;
                        bfr[2][t] = make_uint4(a1, a2, a3, a4);
                    }
                    // six cross products per tap, smallest first: (m,m) (h,l) (l,h) (h,m) (m,h) (h,h)
                    constexpr int pa[6] = {1, 0, 2, 0, 1, 0}, pb[6] = {1, 2, 0, 1, 0, 0};
#pragma unroll
                    for (int p = 0; p < 6; ++p)
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw)
                            acc[kw] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[pa[p]]),
                                                                              __builtin_bit_cast(bf16x8, bfr[kw][pb[p]]), acc[kw], 0, 0, 0);
                }
            }
        }
        row += yb - ya;
    }
    // ---- the wave's three tiles -> this workgroup's partial [tap][output channel][input channel] ----
    float* wp = ws + (((size_t)part * gridDim.y + tile) * 9 + kh * 3) * 1024 + l31;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw)
#pragma unroll
        for (int r = 0; r < 16; ++r) wp[kw * 1024 + ((r & 3) + 8 * (r >> 2) + 4 * half) * 32] = acc[kw][r];
}

// gw[co, ci, tap] = sum over the partials, in their order, in double.  One thread per element of a (padded) tile.
__global__ __launch_bounds__(256) void conv2d_k3_wgrad_sum(const float* __restrict__ ws, float* __restrict__ gw, int C0, int C1, int Cout,
                                                           int nci0, int nci, int nparts, long long per_part) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= per_part) return;
    const int n = (int)(t & 31), m = (int)((t >> 5) & 31);
    const int tt = (int)(t >> 10), tile = tt / 9, tap = tt - tile * 9;
    const int tco = tile / nci, tci = tile - tco * nci;
    const bool second = tci >= nci0;
    const int cl = (second ? tci - nci0 : tci) * 32 + n, co = tco * 32 + m;
    if (cl >= (second ? C1 : C0) || co >= Cout) return;
    const int ci = second ? C0 + cl : cl;
    double s = 0.0;
    for (int p = 0; p < nparts; ++p) s += (double)ws[(size_t)p * per_part + t];
    gw[((size_t)co * (C0 + C1) + ci) * 9 + tap] = (float)s;
}

int k3_check(int B, int C0, int C1, int H, int W, int Cout) {
    SS_REQUIRE(B > 0 && C0 > 0 && C1 >= 0 && H > 0 && W > 0 && Cout > 0);
    // one element's tensors must stay below 2 GiB
    const long long pos4 = (long long)H * W * 4, lim = 1LL << 31;
    if (pos4 * C0 >= lim || pos4 * C1 >= lim || pos4 * Cout >= lim) return SS_ERR_UNSUPPORTED;
    if ((long long)B * H > 0x7fffffffLL) return SS_ERR_UNSUPPORTED;
    if (((long long)ss::ceil_div(C0, 32) + ss::ceil_div(C1, 32)) * ss::ceil_div(Cout, 32) > 65535) return SS_ERR_UNSUPPORTED;
    return SS_OK;
}

}  // namespace

extern "C" int ss_conv2d_k3_wgrad_workspace_bytes(int B, int C0, int C1, int H, int W, int Cout, long long* bytes) {
    SS_REQUIRE(bytes);
    const int status = k3_check(B, C0, C1, H, W, Cout);
    if (status != SS_OK) return status;
    const K3Plan p = k3_plan(B, C0, C1, H, W, Cout);
    *bytes = (long long)p.nparts * p.nci * p.nco * PART * 4;
    return SS_OK;
}

extern "C" int ss_conv2d_k3_wgrad_fwd(const float* grad_out, const float* in0, const float* in1, float* grad_w, float* workspace, int B,
                                      int C0, int C1, int H, int W, int Cout, ss_stream_t stream) {
    SS_REQUIRE(grad_out && in0 && grad_w && workspace);
    SS_REQUIRE(C1 >= 0 && (C1 == 0 || in1));
    const int status = k3_check(B, C0, C1, H, W, Cout);
    if (status != SS_OK) return status;
    const K3Plan p = k3_plan(B, C0, C1, H, W, Cout);
    const int tiles = p.nci * p.nco;
    const long long rows = (long long)B * H, per_part = (long long)tiles * PART;
    hipStream_t st = ss::as_stream(stream);
    hipLaunchKernelGGL(conv2d_k3_wgrad_bf16s, dim3(p.nparts, tiles), dim3(192), 0, st, grad_out, in0, C1 > 0 ? in1 : in0, workspace, C0, C1,
                       H, W, Cout, rows, p.rpp, p.nci0, p.nci);
    int rc = ss::check_launch();
    if (rc != SS_OK) return rc;
    hipLaunchKernelGGL(conv2d_k3_wgrad_sum, dim3((unsigned)ss::ceil_div_ll(per_part, 256)), dim3(256), 0, st, workspace, grad_w, C0, C1,
                       Cout, p.nci0, p.nci, p.nparts, per_part);
    return ss::check_launch();
}
