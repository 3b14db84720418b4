// attention_mass.hip -- Self-Attention Guidance (Hong et al., ICCV 2023): the three launches the method adds around a
// UNet evaluation.
//
//   sdod_attention_mass_f16   mass[b][j] = (1 / heads) sum_h sum_i softmax_i(scale q_h k_h^T)[i][j]: how much softmax probability key j
//                             collects, the one quantity the fused attention kernels never form.  No lq x lk buffer exists anywhere.
//   sdod_sag_degrade_f32      x0 prediction, 9-tap Gaussian blur where the mass says "salient", re-noising: the second UNet's input
//   sdod_sag_fold_f16         the second UNet's prediction folded into the cond rows of the pair prediction, so that every step kernel
//                             produces e_u + g (e_c - e_u) + s (e_u - e_d) unchanged
//
// The mass kernel.  A probability needs its row's normaliser before it can be added into a column, so a workgroup sweeps the keys TWICE
// and recomputes the score tiles in the second sweep instead of storing them:
//   * work split: a workgroup owns 64 query rows of one (batch, head), a wave 16 of them.  The middle map has 64 to a few hundred
//     tokens and 8 heads: 16 .. 100 workgroups, each with its head's whole K in LDS.
//   * K in LDS: while the head's keys fit (128 KiB: 14 tiles of 64 keys at d = 40, 6 at d = 160 -- every middle map up to 384 tokens)
//     all tiles are staged ONCE, zero-padded to the MFMA's K = 32, and both sweeps read them there.  Longer sequences stream the
//     tiles through one stage in both sweeps (two barriers per tile; the second sweep's loads hit L2).
//   * MFMA mapping: S = Q . K^T with the QUERY rows as the A operand (v_mfma_f32_16x16x32_f16), so a lane holds key 16 c + (l & 15)
//     of the tile against queries 4 (l >> 4) + r.  The column sum over a tile's queries is then three in-lane adds and two row
//     swaps (xor 16, xor 32); the per-query maximum and sum of sweep 1 stay lane-local partials over "the keys = l mod 16" and are
//     merged across the 16 lanes once, behind the last tile (a butterfly whose pairs compute the same commutative expression, so
//     the 16 lanes end with the same bits).
//   * sweep 2: p = exp2(s * scale_log2 - m) / l in fp32 (never rounded to fp16: there is no P . V here), summed over the wave's 16
//     queries in registers, over the four waves through LDS in wave order, and written as ONE partial row per workgroup.
//   * reproducibility: partial rows [batch][head][query block][lk] meet in a second launch that adds them in index order and divides
//     by heads.  No atomics; every sum in both launches has a fixed order, so two runs give the same bits.
//   * served, not tuned, at large L: the finishing launch walks heads * nqb partial rows serially per output (8 .. 24 loads at the
//     middle maps SAG uses; 512 dependent loads at lq = lk = 4096 with 8 heads, on B * Lk / 256 workgroups).  A tree over the rows
//     in a fixed order would keep the bits' reproducibility; nothing in the pipeline reaches those sizes yet.
#include "common.h"
#include "sdod_hip.h"
#include "host_util.h"

#include <cmath>

namespace {

constexpr int kMassKT = 64;      // keys per tile
constexpr int kMassQB = 64;      // query rows per workgroup
constexpr int kMassMaxL = 4096;  // the middle map of the largest latents the pipeline builds
constexpr size_t kMassLds = 128 * 1024;

struct MassP {
    const f16* q;
    const f16* k;
    float* part;  // [B * H * nqb][Lk]
    float* mass;  // [B][Lk]
    int B, H, Lq, Lk, ldq, ldk, nqb;
    float scale_log2;
};

template <int D>
constexpr int mass_kstr() { return ((D + 31) / 32) * 32 + 8; } // K tile row stride (halves): the fused attention kernel's
template <int D>
constexpr int mass_resident_tiles() { return (int)(kMassLds / (kMassKT * mass_kstr<D>() * sizeof(f16))); }

template <int D>
__global__ __launch_bounds__(256) void attn_mass_kernel(const MassP p) {
    constexpr int DP = ((D + 31) / 32) * 32, KSTEPS = DP / 32, KSTR = mass_kstr<D>(), KT = kMassKT;
    constexpr int DC = D / 8, DPC = DP / 8, TILE = KT * KSTR;
    static_assert(D % 8 == 0, "head dim must be a multiple of 8");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    f16* smem = reinterpret_cast<f16*>(smem_raw);
    __shared__ float red[2][4][KT]; // a tile's column sums per wave, double-buffered by tile parity: one barrier per tile

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
    const int lid = blockIdx.x; // (batch, head, query block), the partial row's index
    const int bh = lid / p.nqb, qb = lid - bh * p.nqb;
    const int b = bh / p.H, h = bh - b * p.H;
    const int NT = (p.Lk + KT - 1) / KT;
    const bool resident = NT <= mass_resident_tiles<D>(); // (workgroup-uniform)
    const f16* kbase = p.k + (size_t)b * p.Lk * p.ldk + h * D;

    // one K tile into LDS: 16-byte pieces, keys past Lk and columns past D as zeros
    auto stage = [&](int t, f16* dst) {
        for (int idx = tid; idx < KT * DPC; idx += 256) {
            const int row = idx / DPC, ch = idx - row * DPC;
            const int key = t * KT + row;
            const f16x8 v = (key < p.Lk && ch < DC) ? ldg8(kbase + (size_t)key * p.ldk + ch * 8) : zero8();
            *reinterpret_cast<f16x8*>(dst + row * KSTR + ch * 8) = v;
        }
    };
    // Q fragments (A operand: lane = query row l & 15, contraction elements 8 (l >> 4) ..) stay in registers for both sweeps
    f16x8 qf[KSTEPS];
    {
        const int qrow = qb * kMassQB + wave * 16 + li;
        const f16* qp = p.q + ((size_t)b * p.Lq + (qrow < p.Lq ? qrow : 0)) * p.ldq + h * D;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            const int d0 = ks * 32 + g * 8;
            qf[ks] = (qrow < p.Lq && d0 + 8 <= D) ? ldg8(qp + d0) : zero8();
        }
    }
    if (resident) {
        for (int t = 0; t < NT; ++t) stage(t, smem + t * TILE);
        __syncthreads();
    }
    auto tile = [&](int t) -> const f16* {
        if (resident) return smem + t * TILE;
        __syncthreads(); // every wave is done with the previous tile
        stage(t, smem);
        __syncthreads();
        return smem;
    };
    // s[c][r] = q(4 g + r) . k(16 c + li) of tile t; keys past Lk are -inf (m starts finite, so exp2 of them is an exact zero)
    auto scores = [&](const f16* sK, int t, f32x4 (&s)[4]) {
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const f16x8 k8 = *reinterpret_cast<const f16x8*>(sK + (c * 16 + li) * KSTR + ks * 32 + g * 8);
                s[c] = mfma16(qf[ks], k8, s[c]);
            }
        if (t * KT + KT > p.Lk) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (t * KT + c * 16 + li >= p.Lk) s[c] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        }
    };
    const float sc = p.scale_log2;

    // ---- sweep 1: running maximum (scaled, log2 units) and sum of every query, over this lane's keys
    float m[4], l[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { m[r] = -1e30f; l[r] = 0.f; }
    for (int t = 0; t < NT; ++t) {
        const f16* sK = tile(t);
        f32x4 s[4];
        scores(sK, t, s);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float mx = fmaxf(fmaxf(s[0][r], s[1][r]), fmaxf(s[2][r], s[3][r])) * sc; // (scale > 0)
            const float mn = fmaxf(m[r], mx);
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) acc += __builtin_amdgcn_exp2f(__builtin_fmaf(s[c][r], sc, -mn));
            l[r] = __builtin_fmaf(l[r], __builtin_amdgcn_exp2f(m[r] - mn), acc);
            m[r] = mn;
        }
    }
    // merge over the 16 lanes that share the queries; a query past Lq gets weight 0
    float inv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            const float mo = __shfl_xor(m[r], off), lo = __shfl_xor(l[r], off);
            const float mn = fmaxf(m[r], mo);
            // (two rounded products and a sum, never contracted into an fma: that is what makes the pair's results equal)
            l[r] = __fadd_rn(__fmul_rn(l[r], __builtin_amdgcn_exp2f(m[r] - mn)), __fmul_rn(lo, __builtin_amdgcn_exp2f(mo - mn)));
            m[r] = mn;
        }
        inv[r] = (qb * kMassQB + wave * 16 + 4 * g + r < p.Lq) ? 1.0f / l[r] : 0.f;
    }

    // ---- sweep 2: the same scores again, now as probabilities, summed down the query axis
    float* part = p.part + (size_t)lid * p.Lk;
    for (int t = 0; t < NT; ++t) {
        const f16* sK = tile(t);
        f32x4 s[4];
        scores(sK, t, s);
        float cs[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float pr[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) pr[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[c][r], sc, -m[r])) * inv[r];
            cs[c] = quad_rows_sum((pr[0] + pr[1]) + (pr[2] + pr[3])); // over the four 16-lane rows: v_permlane16_swap, v_permlane32_swap
        }
        float(*rd)[KT] = red[t & 1];
        if (g == 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c) rd[wave][c * 16 + li] = cs[c];
        }
        __syncthreads();
        if (tid < KT && t * KT + tid < p.Lk) part[t * KT + tid] = (rd[0][tid] + rd[1][tid]) + (rd[2][tid] + rd[3][tid]);
    }
}

// mass[b][j] = (sum over the image's heads * nqb partial rows, in index order) / heads
__global__ __launch_bounds__(256) void attn_mass_finish_kernel(const MassP p) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.B * p.Lk) return;
    const int b = idx / p.Lk, j = idx - b * p.Lk;
    const int rows = p.H * p.nqb;
    const float* src = p.part + (size_t)b * rows * p.Lk + j;
    float acc = 0.f;
    for (int i = 0; i < rows; ++i) acc += src[(size_t)i * p.Lk];
    p.mass[idx] = acc / (float)p.H;
}

template <int D>
hipError_t mass_launch(const MassP& p, hipStream_t st) {
    constexpr size_t tile_bytes = (size_t)kMassKT * mass_kstr<D>() * sizeof(f16);
    static_assert(mass_resident_tiles<D>() >= 1 && mass_resident_tiles<D>() * tile_bytes <= kMassLds, "LDS");
    static std::atomic<unsigned long long> attr_devs{0};
    if (sdod::first_use_on_device(attr_devs)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_mass_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)kMassLds);
        if (e != hipSuccess) return e;
    }
    const int nt = (p.Lk + kMassKT - 1) / kMassKT;
    const size_t smem = (nt <= mass_resident_tiles<D>() ? nt : 1) * tile_bytes;
    SDOD_LAUNCH((attn_mass_kernel<D>), dim3(p.B * p.H * p.nqb), dim3(256), smem, st, p);
    SDOD_LAUNCH(attn_mass_finish_kernel, dim3((p.B * p.Lk + 255) / 256), dim3(256), 0, st, p);
    return hipGetLastError();
}

bool mass_shape_ok(int batch, int heads, int lq, int lk) {
    return batch >= 1 && batch <= 1024 && heads >= 1 && heads <= 64 && lq >= 1 && lq <= kMassMaxL && lk >= 1 && lk <= kMassMaxL;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// sdod_sag_degrade_f32: a workgroup owns a 32 x 32 tile of one (image, channel) plane.  It forms x0 = (x - b e_u) / a for the tile and
// a 4-pixel halo in LDS, reflect-indexed at the image border, runs the row pass of the 9-tap filter over the 40 haloed rows into a
// second LDS array and the column pass out of that; a pixel keeps x0 unless its middle-map key is salient (mass > 1, strictly).
constexpr int kSagT = 32, kSagR = 4, kSagS = kSagT + 2 * kSagR;
struct SagDegradeP {
    const float* xs;
    const f16* eu;
    const float* mass;
    float* out;
    int n, c, H, W, tiles_x, tiles_y;
    float a, b, ss;
    float w[2 * kSagR + 1];
};
SDOD_DEVICE int sag_reflect(int i, int n) { // one reflection (n >= 8 > halo); positions no output reads are clamped into the image
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}
__global__ __launch_bounds__(256) void sag_degrade_kernel(const SagDegradeP p) {
    __shared__ float x0[kSagS][kSagS + 1], rowp[kSagS][kSagT + 1];
    const int tid = threadIdx.x;
    const int tiles = p.tiles_x * p.tiles_y;
    const int plane = blockIdx.x / tiles, tl = blockIdx.x - plane * tiles;
    const int img = plane / p.c, ch = plane - img * p.c;
    const int ty = tl / p.tiles_x, y0 = ty * kSagT, xb = (tl - ty * p.tiles_x) * kSagT;
    const float* xs = p.xs + (size_t)plane * p.H * p.W;
    const f16* eu = p.eu + (size_t)img * p.H * p.W * p.c + ch;
    for (int idx = tid; idx < kSagS * kSagS; idx += 256) {
        const int ly = idx / kSagS, lx = idx - ly * kSagS;
        const int pix = sag_reflect(y0 + ly - kSagR, p.H) * p.W + sag_reflect(xb + lx - kSagR, p.W);
        x0[ly][lx] = (xs[pix] / p.ss - p.b * (float)eu[(size_t)pix * p.c]) / p.a;
    }
    __syncthreads();
    for (int idx = tid; idx < kSagS * kSagT; idx += 256) {
        const int ly = idx / kSagT, lx = idx - ly * kSagT;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k <= 2 * kSagR; ++k) acc += p.w[k] * x0[ly][lx + k];
        rowp[ly][lx] = acc;
    }
    __syncthreads();
    const int mw = p.W >> 3;
    const float* mass = p.mass + (size_t)img * (p.H >> 3) * mw;
    float* out = p.out + (size_t)plane * p.H * p.W;
    for (int idx = tid; idx < kSagT * kSagT; idx += 256) {
        const int ly = idx / kSagT, lx = idx - ly * kSagT;
        const int gy = y0 + ly, gx = xb + lx;
        if (gy >= p.H || gx >= p.W) continue;
        float d = x0[ly + kSagR][lx + kSagR];
        if (mass[(gy >> 3) * mw + (gx >> 3)] > 1.0f) {
            d = 0.f;
#pragma unroll
            for (int k = 0; k <= 2 * kSagR; ++k) d += p.w[k] * rowp[ly + k][lx];
        }
        const int pix = gy * p.W + gx;
        out[pix] = p.ss * (p.a * d + p.b * (float)eu[(size_t)pix * p.c]);
    }
}

// sdod_sag_fold_f16: cond <- cond + ratio * (uncond - e_d), one fp16 rounding
__global__ __launch_bounds__(256) void sag_fold_kernel(f16* cond, const f16* uncond, const f16* ed, size_t count, float ratio) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    cond[i] = (f16)((float)cond[i] + ratio * ((float)uncond[i] - (float)ed[i]));
}

} // namespace

extern "C" size_t sdod_attention_mass_ws_bytes(int batch, int heads, int lq, int lk) {
    if (!mass_shape_ok(batch, heads, lq, lk)) return 0;
    return (size_t)batch * heads * ((lq + kMassQB - 1) / kMassQB) * lk * sizeof(float);
}

extern "C" int sdod_attention_mass_f16(const void* q, const void* k, float* mass_out, int batch, int heads, int lq, int lk, int d, int ldq,
                                       int ldk, float scale, void* ws, size_t ws_bytes, void* stream) {
    SDOD_TRY
    SDOD_REQUIRE(q && k && mass_out && ws, "null pointer (q, k, mass_out, ws)");
    SDOD_REQUIRE(mass_shape_ok(batch, heads, lq, lk), "bad shape (batch in [1, 1024], heads in [1, 64], lq and lk in [1, 4096])");
    SDOD_REQUIRE(sdod_attention_head_dim_ok(d), "head dim must be one of 40, 64, 80, 160");
    SDOD_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0, "row strides must keep 16-byte alignment");
    SDOD_REQUIRE(ldq >= heads * d && ldk >= heads * d, "row stride < heads*d");
    SDOD_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)ws) & 15) == 0 && ((uintptr_t)mass_out & 3) == 0, "misaligned pointer");
    SDOD_REQUIRE(std::isfinite(scale) && scale > 0.f, "scale must be finite and > 0");
    SDOD_REQUIRE(ws_bytes >= sdod_attention_mass_ws_bytes(batch, heads, lq, lk), "ws_bytes is less than sdod_attention_mass_ws_bytes()");
    MassP p{};
    p.q = (const f16*)q; p.k = (const f16*)k; p.part = (float*)ws; p.mass = mass_out;
    p.B = batch; p.H = heads; p.Lq = lq; p.Lk = lk; p.ldq = ldq; p.ldk = ldk;
    p.nqb = (lq + kMassQB - 1) / kMassQB;
    p.scale_log2 = scale * 1.4426950408889634f;
    hipStream_t st = (hipStream_t)stream;
    switch (d) {
    case 40: SDOD_HIP_CHECK(mass_launch<40>(p, st)); break;
    case 64: SDOD_HIP_CHECK(mass_launch<64>(p, st)); break;
    case 80: SDOD_HIP_CHECK(mass_launch<80>(p, st)); break;
    default: SDOD_HIP_CHECK(mass_launch<160>(p, st)); break;
    }
    return 0;
    SDOD_CATCH
}

extern "C" int sdod_sag_degrade_f32(const float* x_stage, const void* eps_u, const float* mass, float* out, int n, int c, int h, int w,
                                    float a, float b, float stage_scale, const float* taps, void* stream) {
    SDOD_TRY
    SDOD_REQUIRE(x_stage && eps_u && mass && out && taps, "null pointer");
    SDOD_REQUIRE(out != x_stage, "out must not alias x_stage (a tile reads its neighbours' pixels)");
    SDOD_REQUIRE(n >= 1 && n <= 1024 && c >= 1 && c <= 64, "bad shape (n in [1, 1024], c in [1, 64])");
    SDOD_REQUIRE(h >= 8 && w >= 8 && h % 8 == 0 && w % 8 == 0 && h <= 4096 && w <= 4096, "h and w must be multiples of 8 in [8, 4096]");
    SDOD_REQUIRE(std::isfinite(a) && a != 0.f && std::isfinite(b) && std::isfinite(stage_scale) && stage_scale != 0.f,
                 "a and stage_scale must be finite and non-zero, b finite");
    SagDegradeP p{};
    p.xs = x_stage; p.eu = (const f16*)eps_u; p.mass = mass; p.out = out;
    p.n = n; p.c = c; p.H = h; p.W = w;
    p.tiles_x = (w + kSagT - 1) / kSagT; p.tiles_y = (h + kSagT - 1) / kSagT;
    p.a = a; p.b = b; p.ss = stage_scale;
    for (int i = 0; i <= 2 * kSagR; ++i) {
        SDOD_REQUIRE(std::isfinite(taps[i]), "taps must be finite");
        p.w[i] = taps[i];
    }
    const long long blocks = (long long)n * c * p.tiles_x * p.tiles_y;
    SDOD_REQUIRE(blocks <= (1ll << 30), "bad shape (too many tiles)");
    SDOD_LAUNCH(sag_degrade_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    SDOD_HIP_CHECK(hipGetLastError());
    return 0;
    SDOD_CATCH
}

extern "C" int sdod_sag_fold_f16(void* eps_pair, const void* eps_d, size_t count, int uncond_first, float s, float g, void* stream) {
    SDOD_TRY
    SDOD_REQUIRE(eps_pair && eps_d, "null pointer");
    SDOD_REQUIRE(count >= 1 && count <= ((size_t)1 << 36), "bad count");
    SDOD_REQUIRE(std::isfinite(s) && std::isfinite(g) && g != 0.f, "s must be finite, g finite and non-zero");
    const float ratio = s / g;
    SDOD_REQUIRE(std::isfinite(ratio), "s / g must be finite");
    if (ratio == 0.f) return 0; // every bit stays as it was
    f16* lo = (f16*)eps_pair;
    f16* hi = lo + count;
    SDOD_LAUNCH(sag_fold_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, uncond_first ? hi : lo,
                uncond_first ? lo : hi, (const f16*)eps_d, count, ratio);
    SDOD_HIP_CHECK(hipGetLastError());
    return 0;
    SDOD_CATCH
}
