// dense_conv.hip -- the 3x3 convolution of ESRGAN's residual dense block (RRDBNet; sdod_dense_conv3x3_f16, include/sdod_hip.h).
//
// An RDB is five 3x3 convolutions over a growing channel concat (64, 96, 128, 160, 192 input channels).  Here the concat is one wide
// NHWC buffer: the kernel reads channels [0, cin) of every pixel (pixel stride ld_in) and writes its cout channels into a column slice
// of a buffer that may be the same one, with LeakyReLU or the scaled residuals in the epilogue -- so a block needs no concat,
// activation or add launch.
//
// Tiling.  A workgroup (4 waves) owns an 8 x 32 tile of output pixels of one image and all cout channels; wave v owns rows 2v, 2v + 1.
// K is walked in chunks of 32 channels, which every supported cin is a multiple of, so no channel outside [0, cin) is ever read (a
// zero-padded K would multiply whatever those channels hold, and 0 x Inf is NaN).  Per chunk the (8 + 2) x (32 + 2) pixel patch, zero
// outside the image, is staged in LDS -- 340 pixels x 32 halves, pixel stride 40 halves = 80 bytes, which spreads the 16-byte fragment
// reads of 16 consecutive pixels over all 64 banks; the next chunk's patch is fetched into registers while the MFMAs of this one run.
// Each of the nine taps is one K = 32 step of v_mfma_f32_16x16x32_f16 per 16 x 16 block: the weight fragment (A operand, rows = cout)
// comes straight from global memory (the matrix is [cout][9 cin], at most 216 KiB, shared by every workgroup and L2 resident), the
// pixel fragment (B operand) from the patch at the tap's offset.  The accumulator then holds four consecutive output channels of one
// pixel per lane: the epilogue moves 8 bytes per residual read and per store.
// Any n, h, w >= 1 is taken: tiles are clipped at the image edge (patch loads and stores are predicated), so there is no fallback.
#include "common.h"
#include "host_util.h"
#include "sdod_hip.h"

#include <cmath>

namespace {

constexpr int TH = 8, TW = 32, PW = TW + 2, PH = TH + 2, PPIX = PH * PW; // patch: 340 pixels
constexpr int LDP = 40;                                                  // halves per patch pixel (32 + 8 padding)
constexpr int PIECES = PPIX * 4, PITER = (PIECES + 255) / 256;           // 16-byte pieces of a chunk's patch, per-thread count

struct DenseArgs {
    const f16* in;
    const f16* w;
    const float* bias;
    f16* out;         // already offset by out_col
    const f16* res1;
    const f16* res2;
    int ld_in, ld_out, ld_res1, ld_res2;
    int cin, h_in, w_in, ho, wo, ups;
    float alpha, slope, c1;
};

template <int COUT>
__global__ __launch_bounds__(256) void dense_conv_kernel(const DenseArgs a) {
    constexpr int CB = COUT / 16;
    __shared__ __attribute__((aligned(16))) f16 patch[PPIX * LDP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, img = blockIdx.z;
    const f16* in_img = a.in + (size_t)img * a.h_in * a.w_in * a.ld_in;

    // this thread's pieces of the patch: source offset (channel 0 of the chunk) or -1 outside the image
    long long src[PITER];
    int dst[PITER];
#pragma unroll
    for (int i = 0; i < PITER; ++i) {
        const int piece = tid + 256 * i;
        const int pix = piece >> 2, part = piece & 3;
        const int py = pix / PW, px = pix - py * PW;
        const int oy = y0 + py - 1, ox = x0 + px - 1; // output coordinates (before the >> 1 of nearest-2x upsampling)
        const bool ok = piece < PIECES && oy >= 0 && oy < a.ho && ox >= 0 && ox < a.wo;
        src[i] = ok ? ((long long)(oy >> a.ups) * a.w_in + (ox >> a.ups)) * a.ld_in + part * 8 : -1;
        dst[i] = piece < PIECES ? pix * LDP + part * 8 : -1;
    }
    f16x8 stage[PITER];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int i = 0; i < PITER; ++i) stage[i] = src[i] >= 0 ? ldg8(in_img + src[i] + c0) : zero8();
    };

    f32x4 acc[4][CB];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int j = 0; j < CB; ++j) acc[p][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int ldw = 9 * a.cin;
    const f16* wrow = a.w + (size_t)fr * ldw + fg * 8; // weight fragment: row (cout) 16 j + fr, k = 8 fg + e
    // patch pixel of block p (row 2 wave + p / 2, columns 16 (p % 2) + fr) at tap (0, 0)
    int pbase[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) pbase[p] = ((2 * wave + (p >> 1)) * PW + 16 * (p & 1) + fr) * LDP + fg * 8;

    fetch(0);
    for (int c0 = 0; c0 < a.cin; c0 += 32) {
        __syncthreads(); // every wave has finished reading the previous chunk
#pragma unroll
        for (int i = 0; i < PITER; ++i)
            if (dst[i] >= 0) *reinterpret_cast<f16x8*>(&patch[dst[i]]) = stage[i];
        __syncthreads();
        if (c0 + 32 < a.cin) fetch(c0 + 32);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int r = tap / 3, s = tap - 3 * r;
            f16x8 fw[CB], fx[4];
#pragma unroll
            for (int j = 0; j < CB; ++j) fw[j] = ldg8(wrow + (size_t)(16 * j) * ldw + tap * a.cin + c0);
#pragma unroll
            for (int p = 0; p < 4; ++p) fx[p] = *reinterpret_cast<const f16x8*>(&patch[pbase[p] + (r * PW + s) * LDP]);
#pragma unroll
            for (int j = 0; j < CB; ++j)
#pragma unroll
                for (int p = 0; p < 4; ++p) acc[p][j] = mfma16(fw[j], fx[p], acc[p][j]); // lane: pixel fr of block p, channels 16 j + 4 fg + r
        }
    }

    // epilogue: y = alpha (acc + bias); LeakyReLU; + c1 res1; + res2 -- fp32, one rounding
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int oy = y0 + 2 * wave + (p >> 1), ox = x0 + 16 * (p & 1) + fr;
        if (oy >= a.ho || ox >= a.wo) continue;
        const size_t pix = ((size_t)img * a.ho + oy) * a.wo + ox;
#pragma unroll
        for (int j = 0; j < CB; ++j) {
            const int n = 16 * j + 4 * fg;
            const f32x4 b = a.bias ? *reinterpret_cast<const f32x4*>(a.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
            float y[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                y[e] = a.alpha * (acc[p][j][e] + b[e]);
                if (a.slope != 0.f) y[e] = y[e] < 0.f ? a.slope * y[e] : y[e];
            }
            if (a.res1) {
                const f16x4 rv = *reinterpret_cast<const f16x4*>(a.res1 + pix * a.ld_res1 + n);
#pragma unroll
                for (int e = 0; e < 4; ++e) y[e] += a.c1 * (float)rv[e];
            }
            if (a.res2) {
                const f16x4 rv = *reinterpret_cast<const f16x4*>(a.res2 + pix * a.ld_res2 + n);
#pragma unroll
                for (int e = 0; e < 4; ++e) y[e] += (float)rv[e];
            }
            f16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (f16)y[e];
            *reinterpret_cast<f16x4*>(a.out + pix * a.ld_out + n) = o;
        }
    }
}

// How the strided slice [p, p + (pixels - 1) * ld + width) relates to the one at q: 0 = the byte ranges are disjoint; 1 = they share
// pixel rows (same stride, start within one row of each other) on disjoint columns; 2 = the same slice; 3 = anything else.
int slice_relation(const f16* p, long long ld_p, int width_p, const f16* q, long long ld_q, int width_q, long long pixels) {
    const uintptr_t pb = (uintptr_t)p, pe = pb + (size_t)((pixels - 1) * ld_p + width_p) * 2;
    const uintptr_t qb = (uintptr_t)q, qe = qb + (size_t)((pixels - 1) * ld_q + width_q) * 2;
    if (pe <= qb || qe <= pb) return 0;
    if (ld_p != ld_q) return 3;
    if (pb == qb && width_p == width_q) return 2;
    const long long d = ((long long)qb - (long long)pb) / 2; // halves from p to q
    if (d >= 0 && d >= width_p && d + width_q <= ld_p) return 1;
    if (d < 0 && -d >= width_q && -d + width_p <= ld_p) return 1;
    return 3;
}

void dense_conv_require(const sdod_dense_conv_desc* d) {
    SDOD_REQUIRE(d != nullptr, "null descriptor");
    SDOD_REQUIRE(d->in && d->w && d->out, "null pointer (in, w, out)");
    SDOD_REQUIRE((((uintptr_t)d->in | (uintptr_t)d->w | (uintptr_t)d->out | (uintptr_t)d->bias | (uintptr_t)d->res1 | (uintptr_t)d->res2) & 15) == 0,
                 "misaligned pointer (16 bytes)");
    SDOD_REQUIRE(d->cin == 64 || d->cin == 96 || d->cin == 128 || d->cin == 160 || d->cin == 192, "cin must be 64, 96, 128, 160 or 192");
    SDOD_REQUIRE(d->cout == 32 || d->cout == 64, "cout must be 32 or 64");
    SDOD_REQUIRE(d->ld_in >= d->cin && d->ld_in % 8 == 0, "ld_in must be a multiple of 8, at least cin");
    SDOD_REQUIRE(d->ld_out > 0 && d->ld_out % 8 == 0 && d->out_col >= 0 && d->out_col % 8 == 0 && d->out_col + d->cout <= d->ld_out,
                 "ld_out and out_col must be multiples of 8 with out_col + cout <= ld_out");
    SDOD_REQUIRE(!d->res1 || (d->ld_res1 >= d->cout && d->ld_res1 % 8 == 0), "ld_res1 must be a multiple of 8, at least cout");
    SDOD_REQUIRE(!d->res2 || (d->ld_res2 >= d->cout && d->ld_res2 % 8 == 0), "ld_res2 must be a multiple of 8, at least cout");
    SDOD_REQUIRE(d->upsample == 0 || d->upsample == 1, "upsample must be 0 or 1");
    SDOD_REQUIRE(d->n >= 1 && d->n <= 65535 && d->h >= 1 && d->w_in >= 1 && d->h <= 16384 && d->w_in <= 16384, "geometry: n in [1, 65535], h and w in [1, 16384]");
    const long long ho = (long long)d->h << d->upsample, wo = (long long)d->w_in << d->upsample;
    SDOD_REQUIRE((ho + TH - 1) / TH <= 65535 && (long long)d->n * ho * wo < (1ll << 31), "geometry: n * h_out * w_out must stay below 2^31 pixels");
    SDOD_REQUIRE(std::isfinite(d->alpha) && std::isfinite(d->slope) && std::isfinite(d->c1), "alpha, slope and c1 must be finite");
    const long long pin = (long long)d->n * d->h * d->w_in, pout = (long long)d->n * ho * wo;
    const f16* out = (const f16*)d->out + d->out_col;
    // the written slice against the channels read: other workgroups read this pixel's input channels for their halo at any time
    if (d->upsample == 0) {
        const int rel = slice_relation((const f16*)d->in, d->ld_in, d->cin, out, d->ld_out, d->cout, pin);
        SDOD_REQUIRE(rel == 0 || rel == 1, "the written slice overlaps the channels read");
    } else {
        const uintptr_t ib = (uintptr_t)d->in, ie = ib + (size_t)((pin - 1) * d->ld_in + d->cin) * 2;
        const uintptr_t ob = (uintptr_t)out, oe = ob + (size_t)((pout - 1) * d->ld_out + d->cout) * 2;
        SDOD_REQUIRE(oe <= ib || ie <= ob, "the written slice overlaps the input (upsample)");
    }
    // a residual is read at the output pixel by the thread that writes it: the same slice is fine, a partial overlap is not
    if (d->res1) {
        const int rel = slice_relation((const f16*)d->res1, d->ld_res1, d->cout, out, d->ld_out, d->cout, pout);
        SDOD_REQUIRE(rel != 3, "res1 partially overlaps the written slice");
    }
    if (d->res2) {
        const int rel = slice_relation((const f16*)d->res2, d->ld_res2, d->cout, out, d->ld_out, d->cout, pout);
        SDOD_REQUIRE(rel != 3, "res2 partially overlaps the written slice");
    }
}

} // namespace

extern "C" int sdod_dense_conv3x3_ok(const sdod_dense_conv_desc* d) {
    try {
        dense_conv_require(d);
        return 1;
    } catch (...) {
        return 0;
    }
}

extern "C" int sdod_dense_conv3x3_f16(const sdod_dense_conv_desc* d, void* stream) {
    SDOD_TRY
    dense_conv_require(d);
    DenseArgs a;
    a.in = (const f16*)d->in; a.w = (const f16*)d->w; a.bias = d->bias;
    a.out = (f16*)d->out + d->out_col;
    a.res1 = (const f16*)d->res1; a.res2 = (const f16*)d->res2;
    a.ld_in = d->ld_in; a.ld_out = d->ld_out; a.ld_res1 = d->ld_res1; a.ld_res2 = d->ld_res2;
    a.cin = d->cin; a.h_in = d->h; a.w_in = d->w_in; a.ups = d->upsample;
    a.ho = d->h << d->upsample; a.wo = d->w_in << d->upsample;
    a.alpha = d->alpha; a.slope = d->slope; a.c1 = d->c1;
    const dim3 grid((unsigned)((a.wo + TW - 1) / TW), (unsigned)((a.ho + TH - 1) / TH), (unsigned)d->n);
    hipStream_t st = (hipStream_t)stream;
    if (d->cout == 32) SDOD_LAUNCH(dense_conv_kernel<32>, grid, dim3(256), 0, st, a);
    else SDOD_LAUNCH(dense_conv_kernel<64>, grid, dim3(256), 0, st, a);
    SDOD_HIP_CHECK(hipGetLastError());
    return 0;
    SDOD_CATCH
}
