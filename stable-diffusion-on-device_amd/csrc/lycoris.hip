// lycoris.hip -- the LyCORIS families on a packed fp16 weight matrix, in place (include/sdod_hip.h):
//   sdod_loha_merge_f16   W'[row(o)][col(j)] = fp16(float(W) + scale * (sum_r w1a[o][r] w1b[r][j]) * (sum_r w2a[o][r] w2b[r][j]))
//   sdod_lokr_merge_f16   W'[row(o)][col(i, t)] = fp16(fma(scale, float(w1[o / c][i / d]) * float(w2[o % c][i % d][t]), float(W)))
// Both work as lora.hip does: in PACKED coordinates, every access to W a 16-byte one, the factors in canonical PyTorch order and
// the inverse maps (GEGLU row interleave, KRSC columns) applied where the factors are staged or indexed.
//
// LoHa is two of lora.hip's transposed MFMA products (D[j][o] = sum_r b^T[j][r] a^T[r][o], two row-interleaved tiles per
// 32-column block so that a lane holds the 8 consecutive halves of one access) into two accumulator sets, multiplied in fp32.
// The two factor pairs go through the SAME two 64 x 136-half LDS tiles one after the other (34.8 KB, four workgroups per CU as
// the LoRA kernel) rather than through four (69.6 KB, two per CU): the staging of a pair is a few hundred cycles against a
// launch that is bound by its one read and one write of W, and the second pair's global loads need no register the first
// product still holds.  LoKr has no product to stage: a thread owns one 16-byte access of W and indexes w1 / w2 per element.
#include "common.h"
#include "host_util.h"
#include "sdod_hip.h"

#include <cmath>

namespace {

constexpr int kTile = 64;          // rows and columns of W per LoHa workgroup
constexpr int kMaxRank = 128;
constexpr int kLds = kMaxRank + 8; // halves per staged row (lora.hip: the 16 rows of a fragment read start in different banks)

// canonical row of packed row q of an n-row matrix (pack_param_host, PK_LINEAR_GEGLU)
SDOD_DEVICE int canon_row(int n, int geglu, int q) {
    if (!geglu) return q;
    const int within = q & 31, j = (q >> 5) * 16 + (within & 15);
    return within >= 16 ? n / 2 + j : j;
}

struct LohaP {
    f16* w;
    const f16* a[2];  // w1a, w2a: [n][rank]
    const f16* b[2];  // w1b, w2b: [rank][k] ([rank][cin][3][3])
    int n, k, ldw, rank, rp; // rp = rank rounded up to the MFMA K step (32)
    int cin;                 // > 0: 3x3 convolution, packed column t * cin + c <- canonical column c * 9 + t
    int geglu;
    int a_vec[2], b_vec[2];  // the factor can be read 16 bytes at a time
    float scale;
};

// the a tile: rows in packed order, r contiguous; rows >= n and r >= rank are zero
SDOD_DEVICE void stage_a(f16* a_s, const f16* a, int vec, const LohaP& p, int q0, int tid) {
    const int chunks = p.rp / 8;
    for (int idx = tid; idx < kTile * chunks; idx += 256) {
        const int row = idx / chunks, ch = idx - row * chunks;
        const int q = q0 + row;
        f16x8 v = zero8();
        if (q < p.n) {
            const f16* src = a + (size_t)canon_row(p.n, p.geglu, q) * p.rank;
            if (vec) {
                if (ch * 8 < p.rank) v = ldg8(src + ch * 8); // rank % 8 == 0: the chunk is inside the row or past it
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (ch * 8 + e < p.rank) v[e] = src[ch * 8 + e];
            }
        }
        *reinterpret_cast<f16x8*>(&a_s[row * kLds + ch * 8]) = v;
    }
}

// the b tile, transposed: 8 packed columns per thread (k % 8 == 0 and cin % 8 == 0: a chunk never straddles the end of the row
// or a tap), columns >= k and r >= rank are zero
SDOD_DEVICE void stage_b(f16* b_s, const f16* b, int vec, const LohaP& p, int p0, int tid) {
    for (int idx = tid; idx < p.rp * (kTile / 8); idx += 256) {
        const int r = idx / (kTile / 8), ch = idx - r * (kTile / 8);
        const int col = p0 + ch * 8;
        f16x8 v = zero8();
        if (r < p.rank && col < p.k) {
            const f16* src = b + (size_t)r * p.k;
            if (p.cin > 0) {
                const int t = col / p.cin, c = col - t * p.cin;
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = src[(c + e) * 9 + t];
            } else if (vec) {
                v = ldg8(src + col);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = src[col + e];
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) b_s[(ch * 8 + e) * kLds + r] = v[e];
    }
}

// wave w: packed rows 16 w .. + 15 of the tile (the MFMA's columns), all 64 columns (two 32-column blocks); K ascending
SDOD_DEVICE void product(const f16* a_s, const f16* b_s, int rp, int wave, int li, int lg, f32x4 (&acc)[2][2]) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[b][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const f16* a_row = &a_s[(wave * 16 + li) * kLds + 8 * lg];
    for (int ks = 0; ks < rp; ks += 32) {
        const f16x8 bu = *reinterpret_cast<const f16x8*>(a_row + ks);
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int jj = 32 * b + 8 * (li >> 2) + 4 * t + (li & 3);
                const f16x8 ad = *reinterpret_cast<const f16x8*>(&b_s[jj * kLds + 8 * lg + ks]);
                acc[b][t] = mfma16(ad, bu, acc[b][t]);
            }
    }
}

__global__ __launch_bounds__(256) void loha_merge_kernel(const LohaP p) {
    __shared__ __attribute__((aligned(16))) f16 a_s[kTile * kLds]; // [packed row][r]
    __shared__ __attribute__((aligned(16))) f16 b_s[kTile * kLds]; // [packed column][r]
    const int tid = threadIdx.x;
    const int q0 = blockIdx.y * kTile, p0 = blockIdx.x * kTile;
    const int lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    f32x4 acc1[2][2], acc2[2][2];

    stage_a(a_s, p.a[0], p.a_vec[0], p, q0, tid);
    stage_b(b_s, p.b[0], p.b_vec[0], p, p0, tid);
    __syncthreads();
    product(a_s, b_s, p.rp, wave, li, lg, acc1);
    __syncthreads(); // every wave has read the first pair before the second overwrites it
    stage_a(a_s, p.a[1], p.a_vec[1], p, q0, tid);
    stage_b(b_s, p.b[1], p.b_vec[1], p, p0, tid);
    __syncthreads();
    product(a_s, b_s, p.rp, wave, li, lg, acc2);

    // ---- W += scale * p1 * p2: lane (lg, li) holds row q0 + 16 w + li, columns p0 + 32 b + 8 lg .. + 7 (tile t: 4 t .. 4 t + 3)
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
            for (int e = 0; e < 4; ++e) {
                const float had = acc1[b][t][e] * acc2[b][t][e];
                v[4 * t + e] = (f16)fmaf(p.scale, had, (float)v[4 * t + e]);
            }
        stg8(wrow + col, v);
    }
}

struct LokrP {
    f16* w;
    const f16* w1; // [a][b]
    const f16* w2; // [c][d][taps]
    int n, k, ldw;
    int b, c, d;   // w1's columns; w2's rows and input columns
    int cin, taps; // taps == 9: packed column t * cin + i <- canonical (i, t)
    int geglu;
    float scale;
    long long chunks; // n * k / 8
};

// one thread, one 16-byte access of W: 8 consecutive packed columns of a packed row.  They may straddle a w1 column (d % 8 != 0),
// and the rows of a wave a w1 row: everything is indexed per element, from the CANONICAL row and input column.
__global__ __launch_bounds__(256) void lokr_merge_kernel(const LokrP p) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.chunks) return;
    const int cpr = p.k / 8;
    const int q = (int)(idx / cpr), col = (int)(idx - (long long)q * cpr) * 8;
    const int o = canon_row(p.n, p.geglu, q);
    const int o1 = o / p.c, o2 = o - o1 * p.c;
    int t = 0, i = col;
    if (p.taps == 9) { // cin % 8 == 0: the 8 columns share their tap
        t = col / p.cin;
        i = col - t * p.cin;
    }
    int i1 = i / p.d, i2 = i - i1 * p.d;
    const f16* w1row = p.w1 + (size_t)o1 * p.b;
    const f16* w2row = p.w2 + (size_t)o2 * p.d * p.taps + t;
    f16* dst = p.w + (size_t)q * p.ldw + col;
    f16x8 v = ldg8(dst);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (e > 0 && ++i2 == p.d) {
            i2 = 0;
            ++i1;
        }
        const float kr = (float)w1row[i1] * (float)w2row[(size_t)i2 * p.taps]; // 11 x 11 significand bits: exact in fp32
        v[e] = (f16)fmaf(p.scale, kr, (float)v[e]);
    }
    stg8(dst, v);
}

// what the two families share with sdod_lora_merge_f16: the matrix, its column block and its maps
void matrix_require(const void* w, int n, int k, int ldw, float scale, int conv_cin, int geglu) {
    SDOD_REQUIRE(n >= 1 && k >= 8 && k % 8 == 0, "n must be >= 1 and k a positive multiple of 8");
    SDOD_REQUIRE(ldw >= k && ldw % 8 == 0, "ldw must be >= k and a multiple of 8");
    SDOD_REQUIRE(std::isfinite(scale), "scale must be finite");
    SDOD_REQUIRE(reinterpret_cast<uintptr_t>(w) % 16 == 0, "w must be 16-byte aligned");
    SDOD_REQUIRE(conv_cin >= 0 && (conv_cin == 0 || (conv_cin % 8 == 0 && (long long)conv_cin * 9 == k)),
                 "conv_cin must be 0 or a multiple of 8 with k = 9 conv_cin");
    SDOD_REQUIRE(!geglu || n % 32 == 0, "the GEGLU row interleave needs n % 32 == 0");
    SDOD_REQUIRE(!(geglu && conv_cin), "a matrix is either GEGLU-interleaved or a 3x3 convolution");
}

} // namespace

namespace sdod {

void loha_merge_require(const void* w, int n, int k, int ldw, const void* w1a, const void* w1b, const void* w2a, const void* w2b, int rank,
                        float scale, int conv_cin, int geglu) {
    SDOD_REQUIRE(w && w1a && w1b && w2a && w2b, "null pointer");
    SDOD_REQUIRE(rank >= 1 && rank <= kMaxRank, "rank must be in [1, 128]");
    matrix_require(w, n, k, ldw, scale, conv_cin, geglu);
    for (const void* f : {w1a, w1b, w2a, w2b}) SDOD_REQUIRE(reinterpret_cast<uintptr_t>(f) % 2 == 0, "factors must be 2-byte aligned");
}

void lokr_merge_require(const void* w, int n, int k, int ldw, const void* w1, int a, int b, const void* w2, float scale, int conv_cin,
                        int geglu) {
    SDOD_REQUIRE(w && w1 && w2, "null pointer");
    matrix_require(w, n, k, ldw, scale, conv_cin, geglu);
    const int cin = conv_cin > 0 ? conv_cin : k;
    SDOD_REQUIRE(a >= 1 && b >= 1 && n % a == 0 && cin % b == 0, "w1's [a][b] must divide the weight: n % a == 0 and cin % b == 0");
    SDOD_REQUIRE(reinterpret_cast<uintptr_t>(w1) % 2 == 0 && reinterpret_cast<uintptr_t>(w2) % 2 == 0, "factors must be 2-byte aligned");
}

} // namespace sdod

extern "C" int sdod_loha_merge_f16(void* w, int n, int k, int ldw, const void* w1a, const void* w1b, const void* w2a, const void* w2b,
                                   int rank, float scale, int conv_cin, int geglu, void* stream) {
    SDOD_TRY
    sdod::loha_merge_require(w, n, k, ldw, w1a, w1b, w2a, w2b, rank, scale, conv_cin, geglu);
    if (scale == 0.0f) return 0; // W is left bit-identical (a product with -0.0 would not)
    LohaP p{};
    p.w = (f16*)w;
    p.a[0] = (const f16*)w1a; p.b[0] = (const f16*)w1b; p.a[1] = (const f16*)w2a; p.b[1] = (const f16*)w2b;
    p.n = n; p.k = k; p.ldw = ldw; p.rank = rank; p.rp = (rank + 31) / 32 * 32;
    p.cin = conv_cin; p.geglu = geglu ? 1 : 0;
    for (int s = 0; s < 2; ++s) {
        p.a_vec[s] = rank % 8 == 0 && reinterpret_cast<uintptr_t>(p.a[s]) % 16 == 0;
        p.b_vec[s] = reinterpret_cast<uintptr_t>(p.b[s]) % 16 == 0;
    }
    p.scale = scale;
    const unsigned gx = (unsigned)((k + kTile - 1) / kTile), gy = (unsigned)((n + kTile - 1) / kTile);
    SDOD_REQUIRE(gy <= 65535u, "n too large");
    SDOD_LAUNCH(loha_merge_kernel, dim3(gx, gy), dim3(256), 0, (hipStream_t)stream, p);
    SDOD_HIP_CHECK(hipGetLastError());
    return 0;
    SDOD_CATCH
}

extern "C" int sdod_lokr_merge_f16(void* w, int n, int k, int ldw, const void* w1, int a, int b, const void* w2, float scale, int conv_cin,
                                   int geglu, void* stream) {
    SDOD_TRY
    sdod::lokr_merge_require(w, n, k, ldw, w1, a, b, w2, scale, conv_cin, geglu);
    if (scale == 0.0f) return 0;
    LokrP p{};
    p.w = (f16*)w; p.w1 = (const f16*)w1; p.w2 = (const f16*)w2;
    p.n = n; p.k = k; p.ldw = ldw;
    p.cin = conv_cin > 0 ? conv_cin : k; p.taps = conv_cin > 0 ? 9 : 1;
    p.b = b; p.c = n / a; p.d = p.cin / b;
    p.geglu = geglu ? 1 : 0;
    p.scale = scale;
    p.chunks = (long long)n * (k / 8);
    const long long blocks = (p.chunks + 255) / 256;
    SDOD_REQUIRE(blocks <= 0x7fffffffLL, "matrix too large");
    SDOD_LAUNCH(lokr_merge_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    SDOD_HIP_CHECK(hipGetLastError());
    return 0;
    SDOD_CATCH
}
