// attention_wide.hip -- fused softmax(scale * Q K^T) V for ONE head of width 256 or 512 on gfx950: the self-attention in the middle
// of the VAE (Graph::vae_attn_block, C = 4 * vae_channels).  The L x L score matrix never leaves the chip.  DESIGN.md section 6q.
//
// This is not attn_kernel<512>.  At this width one 64-key tile of K or of V alone is 66 KB of LDS, so the two cannot both be
// double-buffered in 160 KB, and a wave's 16 queries x 512 output columns are 128 fp32 accumulators.  The shape of this kernel:
//   * a workgroup of four waves owns 64 query rows, one wave 16 of them and ALL output columns: accumulators (128 registers at
//     d = 512) and the Q fragments (64, scaled once by scale * log2 e) stay in registers for the whole kernel -- one wave per SIMD;
//   * ONE K buffer and ONE V buffer in LDS (134 KB).  The two products alternate, and each buffer is refilled while the OTHER
//     product runs: V(t) is requested from HBM/L2 ahead of Q K^T(t) and stored behind the softmax, K(t + 1) is requested ahead of
//     P V(t) and stored behind it.  Two barriers per tile, 64 staging registers reused by both;
//   * the MFMA mapping of attn_kernel (S^T = K . Q^T, O^T = V^T . P^T, V^T through ds_read_b64_tr_b16): the P registers of a lane
//     are its B operand of the second product, the query stays on the lane, the online rescale is a per-lane multiply;
//   * 64 query blocks at L = 4096 do not fill 256 CUs and a CU holds one workgroup, so where the grid leaves CUs idle -- fewer
//     workgroups than CUs, or a last round that is mostly empty -- the KEYS are split across workgroups: split s runs the same loop
//     over its run of key tiles and parks (m, l, O) in fp32 in a workspace the caller owns, a second small kernel merges the splits.
//     Where the grid already fills its rounds the kernel normalises and stores itself.
#include "common.h"
#include "sdod_hip.h"
#include "host_util.h"

#include <algorithm>
#include <cmath>

namespace {

struct WideP {
    const f16* q;
    const f16* k;
    const f16* v;
    f16* out;
    float* ws; // splits > 1: [B * splits][Lq][D] unnormalised O, then [B * splits][Lq][2] (m in log2 units, l)
    int B, Lq, Lk;
    int ldq, ldk, ldv, ldo;
    float scale_log2;
    int splits, tiles_per_split;
};

typedef short short4v __attribute__((__vector_size__(4 * sizeof(short))));
typedef short short8v __attribute__((__vector_size__(8 * sizeof(short))));
typedef __attribute__((address_space(3))) short4v* lds_short4_ptr;

constexpr int kWideKT = 64;  // keys per tile
constexpr int kWideQB = 64;  // query rows per workgroup
constexpr int kWideCUs = 256; // MI355X
constexpr int kWideMaxSplits = 8;
constexpr int kWideMinTiles = 4; // a split runs at least this many key tiles: the merge reads splits * (D + 2) floats per row

// row strides (halves) of the two LDS tiles: K rows 16 bytes past a multiple of 128 (the b128 operand reads of 16 consecutive
// keys fall into distinct bank groups), V rows 32 * odd bytes (the transposed b64 reads of 4 keys x 16 columns likewise)
constexpr int wide_kstr(int d) { return d + 8; }
constexpr int wide_vstr(int d) { return ((d / 16) | 1) * 16; }
static_assert(wide_vstr(512) == 528 && wide_vstr(256) == 272, "V row stride: the smallest 16 * odd >= d");
constexpr size_t wide_lds_bytes(int d) { return (size_t)kWideKT * (wide_kstr(d) + wide_vstr(d)) * sizeof(f16); }

template <int D>
__global__ __launch_bounds__(256, (D <= 256 ? 2 : 1)) void attn_wide_kernel(const WideP p) {
    constexpr int KSTEPS = D / 32;          // QK^T contraction steps (MFMA K = 32)
    constexpr int NDT = D / 16;             // 16-column output tiles
    constexpr int KSTR = wide_kstr(D), VSTR = wide_vstr(D);
    constexpr int KT = kWideKT;
    constexpr int DC = D / 8;               // 16-byte pieces per K / V row
    constexpr int LD_IT = KT * DC / 256;    // pieces per thread and tile: the staging registers (64 VGPRs at d = 512)
    static_assert(D % 32 == 0 && (KT * DC) % 256 == 0 && 256 % DC == 0, "tile pieces divide evenly over the workgroup");

    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    f16* sK = reinterpret_cast<f16*>(smem_raw);
    f16* sV = sK + KT * KSTR;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, li = lane & 15;

    // 1-D grid, XCD-aware (xcd_remap): the query blocks of one (image, key split) are consecutive logical ids, so the workgroups
    // that stream the same run of K / V rows (17 MB per image at L = 16384, d = 512) sit on one XCD and share its L2
    const int nqb = (p.Lq + kWideQB - 1) / kWideQB;
    const int lid = xcd_remap(blockIdx.x, nqb * p.splits * p.B);
    const int bs = lid / nqb;
    const int b = bs / p.splits, sp = bs - b * p.splits;
    const int q_block = (lid - bs * nqb) * kWideQB;

    const f16* kbase = p.k + (size_t)b * p.Lk * p.ldk;
    const f16* vbase = p.v + (size_t)b * p.Lk * p.ldv;

    // Q fragments, scaled by scale * log2 e once (one more fp16 rounding of Q, no multiply per score): registers for the whole kernel
    const int qrow = q_block + wave * 16 + li;
    f16x8 qf[KSTEPS];
    {
        const f16* qp = p.q + ((size_t)b * p.Lq + (qrow < p.Lq ? qrow : 0)) * p.ldq;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            f16x8 v = qrow < p.Lq ? ldg8(qp + ks * 32 + g * 8) : zero8();
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (f16)((float)v[e] * p.scale_log2);
            qf[ks] = v;
        }
    }

    const int NT = (p.Lk + KT - 1) / KT;
    const int t0 = sp * p.tiles_per_split;
    const int t1 = min(NT, t0 + p.tiles_per_split); // (the launcher leaves no split empty)

    // this thread's pieces of a tile: rows row0 + i * (256 / DC), 16-byte piece ch
    const int row0 = tid / DC, ch = tid - row0 * DC;
    f16x8 stage[LD_IT];
    // (a wave-uniform row pointer plus one 32-bit offset per thread: sixteen per-thread 64-bit addresses for K and as many for V
    // would cost 64 registers)
    auto load_tile = [&](const f16* base, int ld, int t) {
        const unsigned off = (unsigned)row0 * (unsigned)ld + (unsigned)ch * 8u;
        const f16* tile = base + (size_t)t * KT * ld;
        if (t * KT + KT <= p.Lk) { // every tile but a ragged last one: no per-key predicate
#pragma unroll
            for (int i = 0; i < LD_IT; ++i) stage[i] = ldg8(tile + (size_t)(i * (256 / DC)) * ld + off);
            return;
        }
#pragma unroll
        for (int i = 0; i < LD_IT; ++i) { // keys past the sequence: zeros (their P is zero, and zero times garbage need not be)
            const int key = t * KT + row0 + i * (256 / DC);
            stage[i] = key < p.Lk ? ldg8(tile + (size_t)(i * (256 / DC)) * ld + off) : zero8();
        }
    };
    auto store_tile = [&](f16* dst, int stride) {
#pragma unroll
        for (int i = 0; i < LD_IT; ++i) *reinterpret_cast<f16x8*>(dst + (row0 + i * (256 / DC)) * stride + ch * 8) = stage[i];
    };
    // V^T fragment of output tile dt for keys 32 u ..: contraction element e of lane group g is key 32u + 16(e>>2) + 4g + (e&3),
    // the keys whose probabilities the lane holds in pf[u]
    auto read_vt = [&](int u, int dt) -> f16x8 {
        const f16* a0 = sV + (32 * u + 4 * g + (li >> 2)) * VSTR + dt * 16 + 4 * (li & 3);
        const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4_ptr)(a0));
        const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4_ptr)(a0 + 16 * VSTR));
        const short8v both = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        return __builtin_bit_cast(f16x8, both);
    };

    auto read_k = [&](int ks, f16x8 (&f)[4]) { // K fragments of contraction step ks: keys 16 c + li, elements 32 ks + 8 g ..
#pragma unroll
        for (int c = 0; c < 4; ++c) f[c] = *reinterpret_cast<const f16x8*>(sK + (c * 16 + li) * KSTR + ks * 32 + g * 8);
    };
    constexpr int NVG = 2 * NDT / 4; // P V in groups of four MFMAs
    auto read_v = [&](int j, f16x8 (&f)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = read_vt(j / (NDT / 4), (j % (NDT / 4)) * 4 + i);
    };

    f32x4 o[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -1e30f, l_run = 0.f; // running maximum (log2 units) and this lane's share of the running sum

    load_tile(kbase, p.ldk, t0);
    store_tile(sK, KSTR);
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
        // ---- V(t) on its way while S^T = K . Q^T runs: lane gets query li against keys 16 c + 4 g + r
        load_tile(vbase, p.ldv, t);
        f32x4 s[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        // (fragments one step ahead of their MFMAs, and a scheduling fence per step: left alone the scheduler hoists every LDS read
        // of the product to its front -- 256 registers of K fragments at d = 512 -- and spills)
        __builtin_amdgcn_sched_barrier(0);
        f16x8 kf[2][4];
        read_k(0, kf[0]);
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            if (ks + 1 < KSTEPS) read_k(ks + 1, kf[(ks + 1) & 1]);
#pragma unroll
            for (int c = 0; c < 4; ++c) s[c] = mfma16(kf[ks & 1][c], qf[ks], s[c]);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (t * KT + KT > p.Lk) { // the ragged last tile
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (t * KT + c * 16 + g * 4 + r >= p.Lk) s[c][r] = -1e30f;
        }
        // ---- online softmax in the exp2 domain (the scores are already in log2 units)
        float mx = fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3]));
#pragma unroll
        for (int c = 1; c < 4; ++c) mx = fmaxf(mx, fmaxf(fmaxf(s[c][0], s[c][1]), fmaxf(s[c][2], s[c][3])));
        const float m_new = fmaxf(m_run, quad_rows_max(mx));
        // once the maxima have settled no lane of the wave changes its own: skip the 128 accumulator multiplies (wave-uniform)
        const bool rescale = __builtin_amdgcn_ballot_w64(m_new != m_run) != 0;
        const float alpha = rescale ? __builtin_amdgcn_exp2f(m_run - m_new) : 1.0f;
        m_run = m_new;
        float rs = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __builtin_amdgcn_exp2f(s[c][r] - m_new);
                rs += e;
                s[c][r] = e;
            }
        l_run = __builtin_fmaf(l_run, alpha, rs);
        if (rescale) {
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
        }
        f16x8 pf[2];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pf[u][r] = (f16)s[2 * u][r];
                pf[u][4 + r] = (f16)s[2 * u + 1][r];
            }
        store_tile(sV, VSTR);
        __syncthreads(); // V(t) is in LDS, and every wave is done with K(t)
        // ---- K(t + 1) on its way while O^T += V^T . P^T runs
        const bool has_next = t + 1 < t1;
        if (has_next) load_tile(kbase, p.ldk, t + 1);
        __builtin_amdgcn_sched_barrier(0);
        f16x8 vf[2][4];
        read_v(0, vf[0]);
#pragma unroll
        for (int j = 0; j < NVG; ++j) { // group j: key half u = j / (NDT / 4), output tiles 4 (j % (NDT / 4)) .. + 3
            if (j + 1 < NVG) read_v(j + 1, vf[(j + 1) & 1]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int dt = (j % (NDT / 4)) * 4 + i;
                o[dt] = mfma16(vf[j & 1][i], pf[j / (NDT / 4)], o[dt]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (has_next) store_tile(sK, KSTR);
        __syncthreads(); // K(t + 1) is in LDS, and every wave is done with V(t)
    }

    // ---- lane holds O[query qrow][column 16 dt + 4 g + r]
    const float l = quad_rows_sum(l_run);
    if (qrow >= p.Lq) return;
    if (p.splits == 1) {
        const float inv = l > 0.f ? 1.0f / l : 0.f;
        f16* op = p.out + ((size_t)b * p.Lq + qrow) * p.ldo + g * 4;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            f16x4 hv;
#pragma unroll
            for (int r = 0; r < 4; ++r) hv[r] = (f16)(o[dt][r] * inv);
            *reinterpret_cast<f16x4*>(op + dt * 16) = hv;
        }
        return;
    }
    const size_t prow = ((size_t)b * p.splits + sp) * p.Lq + qrow;
    float* wo = p.ws + prow * D + g * 4;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) *reinterpret_cast<f32x4*>(wo + dt * 16) = o[dt];
    if (g == 0) {
        float* wml = p.ws + (size_t)p.B * p.splits * p.Lq * D + prow * 2;
        wml[0] = m_run;
        wml[1] = l;
    }
}

// the splits of one row combined: out = sum_s 2^(m_s - M) O_s / sum_s 2^(m_s - M) l_s.  One thread per (row, four columns).
template <int D>
__global__ __launch_bounds__(256) void attn_wide_merge_kernel(const WideP p) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = idx / (D / 4);
    const int c4 = (int)(idx - row * (D / 4));
    if (row >= (long long)p.B * p.Lq) return;
    const int b = (int)(row / p.Lq), qr = (int)(row - (long long)b * p.Lq);
    const float* ml = p.ws + (size_t)p.B * p.splits * p.Lq * D;
    float M = -1e30f;
    for (int s = 0; s < p.splits; ++s) M = fmaxf(M, ml[(((size_t)b * p.splits + s) * p.Lq + qr) * 2]);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    float den = 0.f;
    for (int s = 0; s < p.splits; ++s) {
        const size_t prow = ((size_t)b * p.splits + s) * p.Lq + qr;
        const float w = __builtin_amdgcn_exp2f(ml[prow * 2] - M);
        den = __builtin_fmaf(w, ml[prow * 2 + 1], den);
        const f32x4 v = *reinterpret_cast<const f32x4*>(p.ws + prow * D + c4 * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = __builtin_fmaf(w, v[r], acc[r]);
    }
    const float inv = den > 0.f ? 1.0f / den : 0.f;
    f16x4 hv;
#pragma unroll
    for (int r = 0; r < 4; ++r) hv[r] = (f16)(acc[r] * inv);
    *reinterpret_cast<f16x4*>(p.out + (size_t)row * p.ldo + c4 * 4) = hv;
}

template <int D>
hipError_t wide_launch(const WideP& p, hipStream_t st) {
    constexpr size_t smem = wide_lds_bytes(D);
    static_assert(smem <= 160 * 1024 && (D > 256 || 2 * smem <= 160 * 1024), "LDS");
    static std::atomic<unsigned long long> attr_devs{0};
    if (sdod::first_use_on_device(attr_devs)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_wide_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return e;
    }
    const int nqb = (p.Lq + kWideQB - 1) / kWideQB;
    SDOD_LAUNCH((attn_wide_kernel<D>), dim3(nqb * p.splits * p.B), dim3(256), smem, st, p);
    if (p.splits > 1) {
        const long long items = (long long)p.B * p.Lq * (D / 4);
        SDOD_LAUNCH((attn_wide_merge_kernel<D>), dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, p);
    }
    return hipGetLastError();
}

// key splits for a shape.  The grid runs in rounds of one workgroup per slot (a CU holds one workgroup at d = 512, two at d = 256), so
// s splits cost ceil(workgroups * s / slots) / s of the unsplit single round: the smallest s within 2 % of the best, if that beats no
// split by 10 %; at most kWideMaxSplits, each at least kWideMinTiles key tiles long, none empty, the workspace at most 256 MiB
int wide_splits(int batch, int lq, int lk, int d, int* tiles_per_split = nullptr) {
    const long long wgs = (long long)((lq + kWideQB - 1) / kWideQB) * batch;
    const int nt = (lk + kWideKT - 1) / kWideKT;
    const long long slots = (long long)kWideCUs * (wide_lds_bytes(d) * 2 <= 160 * 1024 ? 2 : 1);
    auto cost = [&](int s) { return (double)((wgs * s + slots - 1) / slots) / s; };
    const int smax = (int)std::min<long long>(kWideMaxSplits, nt / kWideMinTiles);
    int best = 1;
    for (int s = 2; s <= smax; ++s)
        if ((double)batch * s * lq * (d + 2) * sizeof(float) <= 256.0 * 1024 * 1024 && cost(s) < cost(best) / 1.02) best = s;
    for (int s = 2; s < best; ++s)
        if (cost(s) <= cost(best) * 1.02) { best = s; break; }
    if (cost(best) > cost(1) / 1.1) best = 1;
    const int tps = (nt + best - 1) / best;
    if (tiles_per_split) *tiles_per_split = tps;
    return (nt + tps - 1) / tps;
}

void wide_require_shape(int batch, int lq, int lk, int d) {
    SDOD_REQUIRE(sdod_attention_wide_dim_ok(d), "d must be 256 or 512");
    SDOD_REQUIRE(batch > 0 && batch <= 1024, "batch must be in [1, 1024]");
    SDOD_REQUIRE(lq > 0 && lq <= (1 << 20), "lq must be in [1, 2^20]");
    SDOD_REQUIRE(lk > 0 && lk <= (1 << 20), "lk must be in [1, 2^20]");
    SDOD_REQUIRE((long long)((lq + kWideQB - 1) / kWideQB) * batch <= (1 << 24), "batch * lq too large for one launch");
}

} // namespace

// the widths the wide single-head kernel is instantiated for (4 * vae_channels for vae_channels 64 and 128).  Host-only.
extern "C" int sdod_attention_wide_dim_ok(int d) { return d == 256 || d == 512 ? 1 : 0; }

extern "C" int sdod_attention_wide_splits(int batch, int lq, int lk, int d) {
    if (!sdod_attention_wide_dim_ok(d) || batch <= 0 || lq <= 0 || lk <= 0) return 0;
    return wide_splits(batch, lq, lk, d);
}

extern "C" size_t sdod_attention_wide_ws_bytes(int batch, int lq, int lk, int d) {
    const int s = sdod_attention_wide_splits(batch, lq, lk, d);
    return s > 1 ? (size_t)batch * s * lq * (d + 2) * sizeof(float) : 0;
}

extern "C" int sdod_attention_wide_ws_f16(const void* q, const void* k, const void* v, void* out, int batch, int lq, int lk, int d, int ldq,
                                          int ldk, int ldv, int ldo, float scale, void* ws, size_t ws_bytes, void* stream) {
    SDOD_TRY
    SDOD_REQUIRE(q && k && v && out, "null pointer (q, k, v, out)");
    wide_require_shape(batch, lq, lk, d);
    SDOD_REQUIRE(ldq % 8 == 0 && ldq >= d, "ldq must be a multiple of 8 and >= d");
    SDOD_REQUIRE(ldk % 8 == 0 && ldk >= d, "ldk must be a multiple of 8 and >= d");
    SDOD_REQUIRE(ldv % 8 == 0 && ldv >= d, "ldv must be a multiple of 8 and >= d");
    SDOD_REQUIRE(ldo % 8 == 0 && ldo >= d, "ldo must be a multiple of 8 and >= d");
    SDOD_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 15) == 0, "q, k, v and out must be 16-byte aligned");
    SDOD_REQUIRE(std::isfinite(scale) && scale > 0.f, "scale must be finite and > 0");
    WideP p{};
    p.q = (const f16*)q; p.k = (const f16*)k; p.v = (const f16*)v; p.out = (f16*)out;
    p.B = batch; p.Lq = lq; p.Lk = lk;
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
    p.scale_log2 = scale * 1.4426950408889634f;
    p.tiles_per_split = (lk + kWideKT - 1) / kWideKT;
    p.splits = ws ? wide_splits(batch, lq, lk, d, &p.tiles_per_split) : 1;
    if (p.splits > 1) {
        SDOD_REQUIRE(((uintptr_t)ws & 15) == 0, "ws must be 16-byte aligned");
        SDOD_REQUIRE(ws_bytes >= sdod_attention_wide_ws_bytes(batch, lq, lk, d), "ws_bytes is less than sdod_attention_wide_ws_bytes()");
        p.ws = (float*)ws;
    }
    SDOD_HIP_CHECK(d == 512 ? wide_launch<512>(p, (hipStream_t)stream) : wide_launch<256>(p, (hipStream_t)stream));
    return 0;
    SDOD_CATCH
}

extern "C" int sdod_attention_wide_f16(const void* q, const void* k, const void* v, void* out, int batch, int lq, int lk, int d, int ldq,
                                       int ldk, int ldv, int ldo, float scale, void* stream) {
    return sdod_attention_wide_ws_f16(q, k, v, out, batch, lq, lk, d, ldq, ldk, ldv, ldo, scale, nullptr, 0, stream);
}
