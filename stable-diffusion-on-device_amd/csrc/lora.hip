// lora.hip -- low-rank update of a packed fp16 weight matrix, in place (sdod_lora_merge_f16, include/sdod_hip.h):
//   W'[row(o)][col(j)] = fp16(float(W[row(o)][col(j)]) + scale * sum_r up[o][r] * down[r][j])
// The factors arrive in canonical PyTorch order; row() / col() are the engine's packings (engine.hip: pack_param_host): the
// 16-row value / gate interleave of PK_LINEAR_GEGLU and the KRSC column order of PK_CONV3.  The kernel works in PACKED
// coordinates -- a workgroup owns a 64 x 64 tile of W as it lies in memory -- and applies the inverse maps when it stages
// the factors, so every access to W is a 16-byte one and the maps cost nothing in the product.
//
// The product runs on the matrix cores TRANSPOSED, D[j][o] = sum_r down^T[j][r] up^T[r][o]: the accumulator of
// mfma_f32_16x16x32_f16 has its column on the lane and four consecutive rows in registers, so with W's column index on the
// accumulator rows a lane ends up with consecutive columns of ONE row of W.  Two MFMA tiles whose rows are interleaved in
// groups of four (tile t, row i -> column 8 (i >> 2) + 4 t + (i & 3) of a 32-column block) give every lane the 8 consecutive
// halves of one 16-byte access.  The rank is the MFMA's K: staged zero-padded to a multiple of 32, at most four steps, summed
// in a fixed order -- no atomics, the result is reproducible bit for bit.
#include "common.h"
#include "host_util.h"
#include "sdod_hip.h"

#include <cmath>

namespace {

constexpr int kTile = 64;        // rows and columns of W per workgroup
constexpr int kMaxRank = 128;
constexpr int kLds = kMaxRank + 8; // halves per staged row: 272 bytes, so the 16 rows of a fragment read start in different banks

struct LoraP {
    f16* w;
    const f16* up;
    const f16* down;
    int n, k, ldw, rank, rp; // rp = rank rounded up to the MFMA K step (32)
    int cin;                 // > 0: 3x3 convolution, packed column t * cin + c <- canonical column c * 9 + t
    int geglu;               // packed row (j / 16) * 32 + 16 gate + j % 16 <- canonical row gate * n / 2 + j
    int up_vec, down_vec;    // the factor can be read 16 bytes at a time
    float scale;
};

// canonical row of packed row q (pack_param_host, PK_LINEAR_GEGLU)
SDOD_DEVICE int canon_row(const LoraP& p, int q) {
    if (!p.geglu) return q;
    const int within = q & 31, j = (q >> 5) * 16 + (within & 15);
    return within >= 16 ? p.n / 2 + j : j;
}

__global__ __launch_bounds__(256) void lora_merge_kernel(const LoraP p) {
    __shared__ __attribute__((aligned(16))) f16 up_s[kTile * kLds];   // [packed row][r]
    __shared__ __attribute__((aligned(16))) f16 down_s[kTile * kLds]; // [packed column][r]: the transpose of the down tile
    const int tid = threadIdx.x;
    const int q0 = blockIdx.y * kTile, p0 = blockIdx.x * kTile;
    const int chunks = p.rp / 8;

    // ---- up tile: rows in packed order, r contiguous; rows >= n and r >= rank are zero
    for (int idx = tid; idx < kTile * chunks; idx += 256) {
        const int row = idx / chunks, ch = idx - row * chunks;
        const int q = q0 + row;
        f16x8 v = zero8();
        if (q < p.n) {
            const f16* src = p.up + (size_t)canon_row(p, q) * p.rank;
            if (p.up_vec) {
                if (ch * 8 < p.rank) v = ldg8(src + ch * 8); // rank % 8 == 0: the chunk is inside the row or past it
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (ch * 8 + e < p.rank) v[e] = src[ch * 8 + e];
            }
        }
        *reinterpret_cast<f16x8*>(&up_s[row * kLds + ch * 8]) = v;
    }
    // ---- down tile, transposed: 8 packed columns per thread (k % 8 == 0 and, for a convolution, cin % 8 == 0: a chunk never
    // straddles the end of the row or a tap), columns >= k and r >= rank are zero
    for (int idx = tid; idx < p.rp * (kTile / 8); idx += 256) {
        const int r = idx / (kTile / 8), ch = idx - r * (kTile / 8);
        const int col = p0 + ch * 8;
        f16x8 v = zero8();
        if (r < p.rank && col < p.k) {
            const f16* src = p.down + (size_t)r * p.k;
            if (p.cin > 0) {
                const int t = col / p.cin, c = col - t * p.cin;
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = src[(c + e) * 9 + t];
            } else if (p.down_vec) {
                v = ldg8(src + col);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = src[col + e];
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) down_s[(ch * 8 + e) * kLds + r] = v[e];
    }
    __syncthreads();

    // ---- wave w: packed rows q0 + 16 w .. + 15 (the MFMA's columns), all 64 columns of the tile (two 32-column blocks)
    const int lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    f32x4 acc[2][2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[b][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const f16* up_row = &up_s[(wave * 16 + li) * kLds + 8 * lg];
    for (int ks = 0; ks < p.rp; ks += 32) {
        const f16x8 bu = *reinterpret_cast<const f16x8*>(up_row + ks);
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int jj = 32 * b + 8 * (li >> 2) + 4 * t + (li & 3);
                const f16x8 ad = *reinterpret_cast<const f16x8*>(&down_s[jj * kLds + 8 * lg + ks]);
                acc[b][t] = mfma16(ad, bu, acc[b][t]);
            }
    }

    // ---- W += scale * delta: lane (lg, li) holds row q0 + 16 w + li, columns p0 + 32 b + 8 lg .. + 7 (tile t: 4 t .. 4 t + 3)
    const int q = q0 + wave * 16 + li;
    if (q >= p.n) return;
    f16* wrow = p.w + (size_t)q * p.ldw;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int col = p0 + 32 * b + 8 * lg;
        if (col >= p.k) continue; // nothing past the block's k columns is touched
        f16x8 v = ldg8(wrow + col);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * t + e] = (f16)fmaf(p.scale, acc[b][t][e], (float)v[4 * t + e]);
        stg8(wrow + col, v);
    }
}

} // namespace

namespace sdod {

// the argument checks of sdod_lora_merge_f16, also made by Graph::set_loras for every entry before the arena is touched
void lora_merge_require(const void* w, int n, int k, int ldw, const void* up, const void* down, int rank, float scale, int conv_cin,
                        int geglu) {
    SDOD_REQUIRE(w && up && down, "null pointer");
    SDOD_REQUIRE(rank >= 1 && rank <= kMaxRank, "rank must be in [1, 128]");
    SDOD_REQUIRE(n >= 1 && k >= 8 && k % 8 == 0, "n must be >= 1 and k a positive multiple of 8");
    SDOD_REQUIRE(ldw >= k && ldw % 8 == 0, "ldw must be >= k and a multiple of 8");
    SDOD_REQUIRE(std::isfinite(scale), "scale must be finite");
    SDOD_REQUIRE(reinterpret_cast<uintptr_t>(w) % 16 == 0, "w must be 16-byte aligned");
    SDOD_REQUIRE(reinterpret_cast<uintptr_t>(up) % 2 == 0 && reinterpret_cast<uintptr_t>(down) % 2 == 0, "factors must be 2-byte aligned");
    SDOD_REQUIRE(conv_cin >= 0 && (conv_cin == 0 || (conv_cin % 8 == 0 && (long long)conv_cin * 9 == k)),
                 "conv_cin must be 0 or a multiple of 8 with k = 9 conv_cin");
    SDOD_REQUIRE(!geglu || n % 32 == 0, "the GEGLU row interleave needs n % 32 == 0");
    SDOD_REQUIRE(!(geglu && conv_cin), "a matrix is either GEGLU-interleaved or a 3x3 convolution");
}

} // namespace sdod

extern "C" int sdod_lora_merge_f16(void* w, int n, int k, int ldw, const void* up, const void* down, int rank, float scale,
                                   int conv_cin, int geglu, void* stream) {
    SDOD_TRY
    sdod::lora_merge_require(w, n, k, ldw, up, down, rank, scale, conv_cin, geglu);
    if (scale == 0.0f) return 0; // W is left bit-identical (a product with -0.0 would not)
    LoraP p{};
    p.w = (f16*)w; p.up = (const f16*)up; p.down = (const f16*)down;
    p.n = n; p.k = k; p.ldw = ldw; p.rank = rank; p.rp = (rank + 31) / 32 * 32;
    p.cin = conv_cin; p.geglu = geglu ? 1 : 0;
    p.up_vec = rank % 8 == 0 && reinterpret_cast<uintptr_t>(up) % 16 == 0;
    p.down_vec = reinterpret_cast<uintptr_t>(down) % 16 == 0;
    p.scale = scale;
    const unsigned gx = (unsigned)((k + kTile - 1) / kTile), gy = (unsigned)((n + kTile - 1) / kTile);
    SDOD_REQUIRE(gy <= 65535u, "n too large");
    SDOD_LAUNCH(lora_merge_kernel, dim3(gx, gy), dim3(256), 0, (hipStream_t)stream, p);
    SDOD_HIP_CHECK(hipGetLastError());
    return 0;
    SDOD_CATCH
}
