// attention_kernel.h -- the fused attention kernel (attention.hip has the design notes) and its dispatch, shared by the three files that
// instantiate it: attention.hip (sdod_attention_f16: a sequence is Lk consecutive rows), attention_tiled.hip
// (sdod_attention_tiled_f16: a sequence is one th x tw tile of an h x w token map, walked in place) and attention_shared.hip
// (sdod_attention_shared_f16: a sequence walks its own keys and then an anchor sequence's).  Which of the three is a template
// parameter: TILED changes how a row index becomes an address and nothing else, SHARED which key tiles the loop visits (below).
#pragma once
#include "common.h"
#include "sdod_hip.h"
#include "host_util.h"

#include <climits>
#include <cmath>
#include <cstdlib>
#include <type_traits>

namespace {

struct AttnP {
    const f16* q;
    const f16* k;
    const f16* v;
    f16* out;
    int B, H, Lq, Lk;
    int ldq, ldk, ldv, ldo;
    float scale_log2;
    int causal;
};

// TILED: the sequences are the th x tw tiles of [images][h * w] token maps.  B counts (image, tile) pairs, Lq = Lk = th * tw, and row j
// of a tile is pixel (j / tw) * w + j % tw behind the tile's first one.  The staging threads never divide in the loop: a step of
// 64 * KVS keys moves a key (step_y, step_x) inside the tile, plus one carry when x passes tw.
struct AttnTP : AttnP {
    int w, hw;         // map width; pixels per image
    int th, tw;        // tile sides
    int ntx, ntiles;   // tiles per map row; tiles per image
    int step_y[2], step_x[2]; // (64 * KVS) / tw and (64 * KVS) % tw for KVS = 1, 2
};
// SHARED (attention_shared.hip has the design notes): the last `anchors` of the B sequences are anchor sequences and the B - anchors
// main ones form `anchors` consecutive groups of `per`; a main sequence of group a walks its own Lk keys and then the Lk keys of
// sequence B - anchors + a, and blends the softmax over the first segment with the softmax over both by self_w[a].
struct AttnSP : AttnP {
    int anchors, per;
    const float* self_w; // device memory, [anchors]: read by the kernel, so a captured launch follows the value
};
SDOD_DEVICE int tile_row(const AttnTP& p, int j) {
    const int y = j / p.tw;
    return y * p.w + (j - y * p.tw);
}

typedef short short4v __attribute__((__vector_size__(4 * sizeof(short))));
typedef __attribute__((address_space(3))) short4v* lds_short4_ptr;

constexpr int odd16(int dv) { // smallest 16*odd >= dv  (V row stride in halves: 32*odd bytes, conflict-free tr reads)
    int s = (dv + 15) / 16;
    if ((s & 1) == 0) s += 1;
    return s * 16;
}

// waves per SIMD the register allocation must leave room for: the d = 40 two-query-tile kernel needs 170 VGPRs left alone --
// two over the 168 that let THREE workgroups share a CU (the kernel is issue-bound with stalls a third wave can fill:
// SQ counters, profiles/r02_attention_sq_counters.txt); same step for d = 80 with one query tile (176)
template <int D, int QT>
constexpr int attn_min_waves() { return (D == 40 || (D == 80 && QT == 1)) ? 3 : 1; }

// compile-time loop: f(std::integral_constant<int, 0>{}) ... f(std::integral_constant<int, N - 1>{})
template <int N, int I = 0, class F>
SDOD_DEVICE void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, I + 1>(f);
    }
}

// KVS = key/value split INSIDE the workgroup: KVS groups of four waves own the SAME 64*QT query rows and every KVS-th key tile
// (own LDS stages), and merge their (max, sum, O) through LDS at the end.  For the launches whose grid is one workgroup per CU
// (d = 80 at 32x32: 256 workgroups) the tile loop is a latency-bound chain on one wave per SIMD; a second group halves the
// chain and doubles the waves that hide it, at the same K/V traffic.
template <int D, int QT, bool TR, int KVS = 1, bool TILED = false, bool SHARED = false>
__global__ __launch_bounds__(256 * KVS, (attn_min_waves<D, QT>())) void attn_kernel(
    const std::conditional_t<TILED, AttnTP, std::conditional_t<SHARED, AttnSP, AttnP>> p) {
    static_assert(!(TILED && SHARED), "one variant at a time");
    constexpr int DP = ((D + 31) / 32) * 32; // QK^T contraction, padded to MFMA K=32
    constexpr int KSTEPS = DP / 32;
    constexpr int DV = ((D + 15) / 16) * 16; // PV output columns, padded to 16
    constexpr int NDT = DV / 16;
    constexpr int KSTR = DP + 8;             // K tile row stride (halves)
    constexpr int VSTR = odd16(DV);          // V tile row stride (halves)
    constexpr int KT = 64;                   // keys per tile
    constexpr int DC = D / 8;                // 16-byte chunks per K/V row
    constexpr int LD_IT = (KT * DC + 255) / 256;
    constexpr int STAGE = KT * (KSTR + VSTR);
    // d = 40: V is padded to 48 columns; a column of ones there makes the PV product accumulate the softmax row sum
    // (sum of the SAME fp16-rounded probabilities that weight V) -- 16 packed adds per tile and query tile less on the VALU
    constexpr bool SUM_BY_MFMA = DV > D;
    // d = 40 / 80: the QK^T contraction is padded too (40 -> 64, 80 -> 96); its column D carries the softmax shift into the MFMA.
    // K holds -1 there and Q (prescaled by scale * log2 e) the running shift m, so the MFMA returns s * scale_log2 - m, the
    // exponent itself.  m is DEFERRED: it only has to stay within THR of the true running maximum, which every lane checks on its
    // own scores (a max tree and a wave vote ahead of the exps); only a vote -- and each group's first tile -- takes the exact
    // four-lane maximum, rescales O and writes the new m into Q's column D.  m is held as an fp16 value (it is an MFMA operand),
    // and that exact value is the shift of P, of the rescale and of the KVS merge alike.
    constexpr bool DEFER = DP > D;
    constexpr int KS_M = D / 32, G_M = (D % 32) / 8; // Q fragment (k-step, lane group) that holds contraction element D
    constexpr float THR = 8.0f;                      // log2 units: P <= 2^8 on the common path, far inside fp16
    static_assert(D % 8 == 0, "head dim must be a multiple of 8");

    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int grp = KVS > 1 ? (int)(threadIdx.x >> 8) : 0; // key/value group of this wave (wave-uniform)
    f16* smem = reinterpret_cast<f16*>(smem_raw) + (size_t)grp * 2 * STAGE;

    const int tid = threadIdx.x & 255; // thread inside its group
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int g = lane >> 4;   // lane group 0..3
    const int li = lane & 15;  // index inside the group
    // 1-D grid, XCD-aware: workgroups b and b + 8 share an XCD and its L2 (round-robin dispatch; speed only), so each XCD is
    // handed a contiguous run of logical ids, and the query blocks of one (batch, head) are consecutive ids: the K/V of a
    // head (655 KB at L = 4096, d = 40) is then streamed through ONE L2 instead of all eight (16 heads x 655 KB would thrash
    // every 4 MiB L2 and every K/V tile load would pay the Infinity-Cache round trip)
    const int nqb = (p.Lq + 64 * QT - 1) / (64 * QT);
    const int lid = xcd_remap(blockIdx.x, nqb * p.H * p.B);
    const int bh = lid / nqb;
    const int b = bh / p.H, h = bh - b * p.H;
    const int q_block = (lid - bh * nqb) * (64 * QT);

    // TILED: b is an (image, tile) pair -- the query blocks of one (image, tile, head) are consecutive logical ids just the same, so
    // a tile's K/V stream through one L2 -- and row0 the tile's first pixel, in rows of the token map; there is no causal form
    const int causal = (TILED || SHARED) ? 0 : p.causal;
    size_t row0 = 0;
    if constexpr (TILED) {
        const int img = b / p.ntiles, tl = b - img * p.ntiles;
        const int ty = tl / p.ntx, tx = tl - ty * p.ntx;
        row0 = (size_t)img * p.hw + (size_t)(ty * p.th) * p.w + tx * p.tw;
    }
    const f16* kbase = p.k + (TILED ? row0 : (size_t)b * p.Lk) * p.ldk + h * D;
    const f16* vbase = p.v + (TILED ? row0 : (size_t)b * p.Lk) * p.ldv + h * D;

    // SHARED: this workgroup's blend weight and where its second key segment lies, in rows behind its own first key (the anchors
    // are the last sequences: never negative).  All of it is workgroup-uniform: w == 1 and the anchor sequences themselves walk one
    // segment -- the plain kernel's loop, bit for bit -- and w == 0 walks two without a snapshot.
    float self_w = 1.f;
    size_t seg_rows = 0;
    if constexpr (SHARED) {
        const int nmain = p.B - p.anchors;
        if (b < nmain) {
            const int ga = b / p.per;
            self_w = p.self_w[ga];
            seg_rows = (size_t)(nmain + ga - b) * p.Lk;
        }
    }
    const bool two_segments = SHARED && self_w != 1.f;
    const bool blend = two_segments && self_w != 0.f;

    // zero the padded columns of both stages once (they are never overwritten by the staging stores)
    {
        constexpr int KPADC = (DP - D) / 8, VPADC = (DV - D) / 8;
        for (int st = 0; st < 2; ++st) {
            f16* sK = smem + st * STAGE;
            f16* sV = sK + KT * KSTR;
            if (KPADC > 0)
                for (int idx = tid; idx < KT * KPADC; idx += 256) {
                    const int row = idx / (KPADC > 0 ? KPADC : 1), ch = idx - row * KPADC;
                    f16x8 pad = zero8();
                    if (DEFER && ch == 0) pad[0] = (f16)-1.0f; // column D: minus the shift held in Q's column D
                    *reinterpret_cast<f16x8*>(sK + row * KSTR + D + ch * 8) = pad;
                }
            if (VPADC > 0)
                for (int idx = tid; idx < KT * VPADC; idx += 256) {
                    const int row = idx / (VPADC > 0 ? VPADC : 1), ch = idx - row * VPADC;
                    f16x8 pad = zero8();
                    if (ch == 0) pad[0] = (f16)1.0f; // column D: the row-sum column (SUM_BY_MFMA)
                    *reinterpret_cast<f16x8*>(sV + row * VSTR + D + ch * 8) = pad;
                }
        }
    }

    // Q fragments stay in registers for the whole kernel
    f16x8 qf[QT][KSTEPS];
    int qrow[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        qrow[t] = q_block + wave * (16 * QT) + t * 16 + li;
        const f16* qp; // (TILED: the row map, once per workgroup; rows past Lq make an address nothing reads)
        if constexpr (TILED) qp = p.q + (row0 + tile_row(p, qrow[t])) * p.ldq + h * D;
        else qp = p.q + ((size_t)b * p.Lq + qrow[t]) * p.ldq + h * D;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            const int d0 = ks * 32 + g * 8;
            qf[t][ks] = (qrow[t] < p.Lq && d0 + 8 <= D) ? ldg8(qp + d0) : zero8();
            if (DEFER) // the softmax scale (log2 units) folded into Q once: one more fp16 rounding of Q, no per-score multiply
#pragma unroll
                for (int e = 0; e < 8; ++e) qf[t][ks][e] = (f16)((float)qf[t][ks][e] * p.scale_log2);
        }
    }

    int kend = p.Lk;
    if (causal) kend = min(p.Lk, q_block + 64 * QT);
    const int NT = (kend + KT - 1) / KT;

    f16x8 rk[LD_IT], rv[LD_IT];
    const f16* kptr0[LD_IT];
    const f16* vptr0[LD_IT]; // this thread's 16-byte pieces of key tile 0 (TILED: unused)
    // TILED: where this thread's pieces of the NEXT key tile to load lie -- byte offsets behind kbase / vbase (32 bits: the host
    // bounds them) and the key's column inside the tile.  The group's tiles are loaded in order (grp, grp + KVS, ...), so each
    // load_tile ends by moving its pieces 64 * KVS keys on: step_y rows and step_x columns, one more row where x passes tw.
    unsigned kofs[TILED ? LD_IT : 1], vofs[TILED ? LD_IT : 1];
    int kx[TILED ? LD_IT : 1];
#pragma unroll
    for (int i = 0; i < LD_IT; ++i) {
        const int idx = tid + 256 * i;
        const int row = idx / DC, ch = idx - row * DC;
        if constexpr (TILED) {
            const int j = grp * KT + row, y = j / p.tw;
            kx[i] = j - y * p.tw;
            kofs[i] = (unsigned)(((y * p.w + kx[i]) * p.ldk + ch * 8) * (int)sizeof(f16));
            vofs[i] = (unsigned)(((y * p.w + kx[i]) * p.ldv + ch * 8) * (int)sizeof(f16));
        } else {
            kptr0[i] = kbase + (size_t)row * p.ldk + ch * 8;
            vptr0[i] = vbase + (size_t)row * p.ldv + ch * 8;
        }
    }
    // t: the tile inside its segment; seg: the segment's first key, in rows behind kbase / vbase (SHARED: the anchor's; else 0)
    auto load_tile = [&](int t, size_t seg = 0) {
        if constexpr (TILED) {
            auto at = [](const f16* base, unsigned bytes) { return reinterpret_cast<const f16*>(reinterpret_cast<const char*>(base) + bytes); };
            // the same two forms as below: a tile inside the sequence loads unpredicated, a ragged one zero-fills key by key
            const bool full = t * KT + KT <= p.Lk;
            const int sx = p.step_x[KVS - 1];
            const unsigned row_pix = (unsigned)(p.step_y[KVS - 1] * p.w + sx), wrap_pix = (unsigned)(p.w - p.tw);
            const unsigned ks0 = row_pix * p.ldk * 2u, ks1 = ks0 + wrap_pix * p.ldk * 2u; // wave-uniform steps, without and with the carry
            const unsigned vs0 = row_pix * p.ldv * 2u, vs1 = vs0 + wrap_pix * p.ldv * 2u;
#pragma unroll
            for (int i = 0; i < LD_IT; ++i) {
                const int idx = tid + 256 * i;
                if (full) {
                    if (idx < KT * DC) {
                        rk[i] = ldg8(at(kbase, kofs[i]));
                        rv[i] = ldg8(at(vbase, vofs[i]));
                    }
                } else {
                    const bool ok = (idx < KT * DC) && (t * KT + idx / DC < p.Lk);
                    rk[i] = ok ? ldg8(at(kbase, kofs[i])) : zero8();
                    rv[i] = ok ? ldg8(at(vbase, vofs[i])) : zero8();
                }
                const int x = kx[i] + sx;
                const bool carry = x >= p.tw;
                kx[i] = carry ? x - p.tw : x;
                kofs[i] += carry ? ks1 : ks0;
                vofs[i] += carry ? vs1 : vs0;
            }
            return;
        }
        // A tile that lies entirely inside the sequence (every tile but a ragged last one) needs no per-key predicate and no
        // zero fill: the lanes past the tile's 16-byte pieces keep whatever their registers hold -- store_tile skips them.
        // (The predicated form costs a compare, an exec dance and eight register clears per piece: ~10 % of the loop's VALU.)
        if (t * KT + KT <= p.Lk) {
            const size_t ko = ((size_t)t * KT + seg) * p.ldk, vo = ((size_t)t * KT + seg) * p.ldv; // wave-uniform: one 64-bit add per load
#pragma unroll
            for (int i = 0; i < LD_IT; ++i) {
                if (tid + 256 * i < KT * DC) {
                    rk[i] = ldg8(kptr0[i] + ko);
                    rv[i] = ldg8(vptr0[i] + vo);
                }
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < LD_IT; ++i) {
            const int idx = tid + 256 * i;
            const int row = idx / DC, ch = idx - row * DC;
            const int key = t * KT + row;
            const bool ok = (idx < KT * DC) && (key < p.Lk);
            rk[i] = ok ? ldg8(kbase + (seg + key) * p.ldk + ch * 8) : zero8();
            rv[i] = ok ? ldg8(vbase + (seg + key) * p.ldv + ch * 8) : zero8();
        }
    };
    auto store_tile = [&](int st) {
        f16* sK = smem + st * STAGE;
        f16* sV = sK + KT * KSTR;
#pragma unroll
        for (int i = 0; i < LD_IT; ++i) {
            const int idx = tid + 256 * i;
            const int row = idx / DC, ch = idx - row * DC;
            if (idx < KT * DC) {
                *reinterpret_cast<f16x8*>(sK + row * KSTR + ch * 8) = rk[i];
                *reinterpret_cast<f16x8*>(sV + row * VSTR + ch * 8) = rv[i];
            }
        }
    };

    f32x4 o[QT][NDT];
    float m_run[QT], l_run[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        m_run[t] = DEFER ? 0.f : -1e30f; // (DEFER: the zero Q column D holds; the first tile sets m whatever it is)
        l_run[t] = 0.f;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) o[t][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

#ifdef SDOD_ATTN_ABLATE
    constexpr int abl = SDOD_ATTN_ABLATE; // developer builds only (make lib/libsdod_attnabl<mask>.so): 1 = no K/V loads after tile 0,
#else                                     // 2 = no exp in the softmax; results are wrong, only the timing is of interest
    constexpr int abl = 0;
#endif
    constexpr bool HOLD = D <= 80; // K / V^T fragments of a tile are read once and kept for both query tiles (d = 160: read at the point of use)
    auto read_vt = [&](const f16* sV, int u, int dt) -> f16x8 {
        const f16* a0 = sV + (32 * u + 4 * g + (li >> 2)) * VSTR + dt * 16 + 4 * (li & 3);
        const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4_ptr)(a0));
        const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4_ptr)(a0 + 16 * VSTR));
        typedef short short8v __attribute__((__vector_size__(8 * sizeof(short))));
        const short8v both = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        return __builtin_bit_cast(f16x8, both);
    };
    // ---- online softmax of query tile A against key tile t (scores in s_a) and O^T += V^T . P^T; lane owns query qrow[A],
    // keys t*64 + c*16 + 4g + r.  VALU budget matters here (at d=40 the MFMAs of a tile take ~450 cycles, a naive softmax 3x
    // that): DEFER (d = 40 / 80) the MFMA already returned the exponent, the common path is a lane-local max tree, a vote and
    // one v_exp per score; otherwise the row max is taken on the RAW scores (scale > 0) and exp2(s*c - m*c) is one fma + one
    // v_exp.  Masking code only runs for tiles that contain masked keys (the last ragged tile / the causal diagonal).
    // thr (DEFER only): the vote threshold's bit pattern, INT_MIN on a group's first tile.
    auto softmax_pv = [&](auto a_c, int t, int thr, f32x4 (&s_a)[4], const f16x8 (&vfr)[HOLD ? 2 : 1][HOLD ? NDT : 1],
                          const f16* sV) {
        constexpr int a = decltype(a_c)::value;
        const bool need_mask = (t * KT + KT > p.Lk) || (causal && (t * KT + KT - 1 > q_block + wave * (16 * QT)));
        if (need_mask) {
            // (key0 goes through an opaque statement so that the sixteen key indices are computed INSIDE this rarely taken
            // branch: the compiler otherwise hoists them in front of it and every tile pays for them)
            int key0 = t * KT + g * 4;
            asm volatile("" : "+v"(key0));
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = key0 + c * 16 + r;
                    const bool masked = (key >= p.Lk) | (causal & (key > qrow[a]));
                    s_a[c][r] = masked ? -1e30f : s_a[c][r];
                }
        }
        // row maximum of this lane's 16 scores: three-input maxima (v_max3_f32: 8 instructions instead of 15) as a TREE of depth 3,
        // not a chain of 8 -- the maximum heads the tile's dependent chain (max -> exp -> PV)
        auto lane_max = [&]() {
            const float t0 = fmaxf(fmaxf(s_a[0][0], s_a[0][1]), s_a[0][2]);
            const float t1 = fmaxf(fmaxf(s_a[0][3], s_a[1][0]), s_a[1][1]);
            const float t2 = fmaxf(fmaxf(s_a[1][2], s_a[1][3]), s_a[2][0]);
            const float t3 = fmaxf(fmaxf(s_a[2][1], s_a[2][2]), s_a[2][3]);
            const float t4 = fmaxf(fmaxf(s_a[3][0], s_a[3][1]), s_a[3][2]);
            const float u0 = fmaxf(fmaxf(t0, t1), t2);
            const float u1 = fmaxf(fmaxf(t3, t4), s_a[3][3]);
            return fmaxf(u0, u1);
        };
        float rs[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (DEFER) {
            // s_a = s * scale_log2 - m already.  Vote: does any score of the wave exceed m by more than THR?  The lane's maximum
            // is taken on the bit patterns as signed integers (v_max3_i32): exact for the comparison against a positive
            // threshold (every negative float is a negative integer) and free of the canonicalising moves fmaxf costs on MFMA
            // results.  On a group's first tile (thr = INT_MIN) every wave takes the branch.
            auto bi = [](float x) { return __builtin_bit_cast(int, x); };
            auto mx3 = [](int x, int y, int z) { return max(max(x, y), z); };
            const int t0 = mx3(bi(s_a[0][0]), bi(s_a[0][1]), bi(s_a[0][2]));
            const int t1 = mx3(bi(s_a[0][3]), bi(s_a[1][0]), bi(s_a[1][1]));
            const int t2 = mx3(bi(s_a[1][2]), bi(s_a[1][3]), bi(s_a[2][0]));
            const int t3 = mx3(bi(s_a[2][1]), bi(s_a[2][2]), bi(s_a[2][3]));
            const int t4 = mx3(bi(s_a[3][0]), bi(s_a[3][1]), bi(s_a[3][2]));
            const int mi = max(mx3(t0, t1, t2), mx3(t3, t4, bi(s_a[3][3])));
            if (__builtin_amdgcn_ballot_w64(mi > thr) != 0) {
                const bool first = thr == INT_MIN;
                // rare (and each group's first tile): the exact maximum of the query's 64 scores, a new shift rounded to fp16,
                // O (and at d = 80 the row sum) rescaled to it, Q's column D updated for the next tiles, and THIS tile's
                // exponents re-based BEFORE any exp2 of it is taken -- nothing computed at the old shift reaches P . V
                const float mx = quad_rows_max(lane_max());
                const float m_old = m_run[a];
                float m_new = m_old;
                if (first || mx > 0.f) m_new = (float)(f16)fminf(fmaxf(m_old + mx, -65504.f), 65504.f);
                const float delta = m_new - m_old;
                if (!first) { // (O and l are still zero on the first tile)
                    const float alpha = __builtin_amdgcn_exp2f(-delta);
#pragma unroll
                    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) o[a][dt][r] *= alpha;
                    if (!SUM_BY_MFMA) l_run[a] *= alpha;
                }
                m_run[a] = m_new;
                if (g == G_M) qf[a][KS_M][0] = (f16)m_new;
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r) s_a[c][r] -= delta;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = s_a[c][r];
                    if (!(abl & 2)) v = __builtin_amdgcn_exp2f(v);
                    if (!SUM_BY_MFMA) rs[r] += v;
                    s_a[c][r] = v;
                }
            }
            if (!SUM_BY_MFMA) l_run[a] += (rs[0] + rs[1]) + (rs[2] + rs[3]);
        } else {
            // the four lanes that share a query: row swaps in VALU latency instead of two ds_bpermute round trips on the loop's
            // critical path (common.h: quad_rows_max; profiles/r03_attention_permlane.txt)
            const float mx = quad_rows_max(lane_max());
            const float m_new = fmaxf(m_run[a], mx * p.scale_log2); // running max in scaled (log2) units
            // once the running maxima have settled (a few tiles in) no lane of the wave changes its maximum: skip the
            // rescale of the output accumulators (wave-uniform branch)
            const bool rescale = __builtin_amdgcn_ballot_w64(m_new != m_run[a]) != 0;
            const float alpha = rescale ? __builtin_amdgcn_exp2f(m_run[a] - m_new) : 1.0f;
            m_run[a] = m_new;
            // plain fp32 fma / add, NOT the packed forms: beside MFMAs a v_pk_add_f32 / v_pk_fma_f32 costs several times the
            // issue cycles of the two scalar instructions it replaces (MI355X_MICROARCH.md, per-instruction constants: an
            // anti-lever), and this loop is bound by the SIMD's vector issue (-ffp-contract=off: the fma is spelled out)
            const float sc = p.scale_log2, nm = -m_new;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = __builtin_fmaf(s_a[c][r], sc, nm);
                    if (!(abl & 2)) v = __builtin_amdgcn_exp2f(v);
                    if (!SUM_BY_MFMA) rs[r] += v;
                    s_a[c][r] = v;
                }
            }
            if (!SUM_BY_MFMA) l_run[a] = __builtin_fmaf(l_run[a], alpha, (rs[0] + rs[1]) + (rs[2] + rs[3]));
            if (rescale) {
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[a][dt][r] *= alpha;
            }
        }
        f16x8 pf[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            f16x8 f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                f[r] = (f16)s_a[2 * u][r];
                f[4 + r] = (f16)s_a[2 * u + 1][r];
            }
            pf[u] = f;
        }
        // ---- O^T += V^T . P^T for this query tile; contraction element e of lane group g is key 32u + 16(e>>2) + 4g + (e&3)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                f16x8 vf;
                if (TR) {
                    vf = HOLD ? vfr[u][dt] : read_vt(sV, u, dt);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) vf[e] = sV[(32 * u + 16 * (e >> 2) + 4 * g + (e & 3)) * VSTR + dt * 16 + li];
                }
                o[a][dt] = mfma16(vf, pf[u], o[a][dt]);
            }
        }
    };
    auto read_k = [&](const f16* sK, f16x8 (&kf)[HOLD ? KSTEPS : 1][4]) {
        if constexpr (HOLD) {
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks)
#pragma unroll
                for (int c = 0; c < 4; ++c) kf[ks][c] = *reinterpret_cast<const f16x8*>(sK + (c * 16 + li) * KSTR + ks * 32 + g * 8);
        }
    };
    auto read_v = [&](const f16* sV, f16x8 (&vfr)[HOLD ? 2 : 1][HOLD ? NDT : 1]) {
        if constexpr (TR && HOLD) {
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) vfr[u][dt] = read_vt(sV, u, dt);
        }
    };
    // S^T = K . Q^T of one key tile for every query tile of the wave
    auto qk = [&](const f16* sK, const f16x8 (&kf)[HOLD ? KSTEPS : 1][4], f32x4 (&s)[QT][4]) {
#pragma unroll
        for (int a = 0; a < QT; ++a) {
#pragma unroll
            for (int c = 0; c < 4; ++c) s[a][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const f16x8 k8 = HOLD ? kf[ks][c] : *reinterpret_cast<const f16x8*>(sK + (c * 16 + li) * KSTR + ks * 32 + g * 8);
                    s[a][c] = mfma16(k8, qf[a][ks], s[a][c]);
                }
        }
    };

    // (Round 3 tried a software-pipelined form of this loop -- the scores of tile t + 1 computed under the softmax of tile t,
    // three LDS stages, K fragments read behind the previous barrier: 220 VGPRs, 8 % SLOWER (123 vs 113 us at 4096^2, d = 40:
    // the compiler serialises the longer body no better, and the third LDS stage costs occupancy where B >= 4 would have
    // used it).  Removed; profiles/r03_attention_occupancy.txt keeps the numbers.)
    if (grp < NT) {
        load_tile(grp);
        store_tile(0);
    }
    __syncthreads();
    const int NTG = (NT + KVS - 1) / KVS; // every group runs the same number of iterations (the barriers are workgroup-wide)
    int thr = INT_MIN;                    // DEFER: the vote threshold of softmax_pv (INT_MIN: a group's first tile)
    // SHARED: the segments are walked one after the other, NTG rounds each, and EACH is dealt to the groups from its own tile 0, so
    // that every group stands at the segment boundary in the same round (it == NTG) and the blend's snapshot is taken there.  t
    // counts inside the segment -- the ragged tile and its mask are the segment's -- and seg moves the loads to the anchor's rows.
    // thr stays INT_MIN until the group has really run a tile: with one tile per segment, group 1's first is the anchor's.
    const int NIT = two_segments ? 2 * NTG : NTG;
    // SHARED, 0 < w < 1: w * (the normalised softmax over the own segment), parked in the workgroup's OWN output rows as fp16 -- every
    // lane writes the pieces it will overwrite in the epilogue and reads them back there itself, so the snapshot costs no LDS and no
    // register across the anchor segment, and nothing at all where blend is false (DESIGN.md 6t weighs the alternatives).
    auto snapshot_store = [&](int a, float l, auto&& value) {
        const float f = l > 0.f ? self_w / l : 0.f;
        if (qrow[a] < p.Lq) {
            f16* op = p.out + ((size_t)b * p.Lq + qrow[a]) * p.ldo + h * D;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                const int dv0 = dt * 16 + g * 4;
                if (dv0 < D) {
                    f16x4 hv;
#pragma unroll
                    for (int r = 0; r < 4; ++r) hv[r] = (f16)(value(dt, r) * f);
                    *reinterpret_cast<f16x4*>(op + dv0) = hv;
                }
            }
        }
    };
    auto snapshot = [&](int it) {
        if constexpr (KVS == 1) {
#pragma unroll
            for (int a = 0; a < QT; ++a) {
                const float l = SUM_BY_MFMA ? __shfl(o[a][D / 16][D % 4], ((D % 16) / 4) * 16 + li) : quad_rows_sum(l_run[a]);
                snapshot_store(a, l, [&](int dt, int r) { return o[a][dt][r]; });
            }
        } else {
            // two groups: the own segment's softmax is the merge of their states.  Group 1 parks its (m, l, O) in the stage it read
            // last round (free since that round's barrier; the round's prefetch went to the other one), group 0 combines them on the
            // fly without touching its own state, and a second barrier keeps group 1's next store_tile behind group 0's reads.
            static_assert(QT == 1 && !SUM_BY_MFMA, "the key/value split runs d = 80 with one query tile");
            static_assert((size_t)(2 + NDT * 4) * 256 * sizeof(float) <= (size_t)STAGE * sizeof(f16), "snapshot merge fits one stage");
            float* mrg = reinterpret_cast<float*>(reinterpret_cast<f16*>(smem_raw) + (size_t)(2 + ((it & 1) ^ 1)) * STAGE);
            if (grp == 1) {
                mrg[0 * 256 + tid] = m_run[0];
                mrg[1 * 256 + tid] = l_run[0];
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) mrg[(2 + dt * 4 + r) * 256 + tid] = o[0][dt][r];
            }
            __syncthreads();
            if (grp == 0) {
                const float m1 = mrg[0 * 256 + tid], l1 = mrg[1 * 256 + tid];
                const float m = fmaxf(m_run[0], m1);
                const float a0 = __builtin_amdgcn_exp2f(m_run[0] - m), a1 = __builtin_amdgcn_exp2f(m1 - m);
                const float l = quad_rows_sum(l_run[0] * a0 + l1 * a1);
                snapshot_store(0, l, [&](int dt, int r) { return o[0][dt][r] * a0 + mrg[(2 + dt * 4 + r) * 256 + tid] * a1; });
            }
            __syncthreads();
            // the merge ran over the stage's padded K columns, which no store_tile writes: group 1 sets them again (V has none at
            // d = 80); its next store_tile into the stage and the reads behind this round's barrier find them as the prologue left them
            static_assert(DV == D && DEFER, "the lent stage has padded K columns only");
            if (grp == 1) {
                constexpr int KPADC = (DP - D) / 8;
                f16* sK = smem + ((it & 1) ^ 1) * STAGE;
                for (int idx = tid; idx < KT * KPADC; idx += 256) {
                    const int row = idx / KPADC, ch = idx - row * KPADC;
                    f16x8 pad = zero8();
                    if (ch == 0) pad[0] = (f16)-1.0f;
                    *reinterpret_cast<f16x8*>(sK + row * KSTR + D + ch * 8) = pad;
                }
            }
        }
    };
    for (int it = 0; it < NIT; ++it) {
        const bool anchor_seg = SHARED && it >= NTG;
        const int t = (anchor_seg ? it - NTG : it) * KVS + grp;
        const int cur = it & 1;
        // the tile this group runs in the next round
        int t_next = t + KVS;
        size_t seg_next = 0;
        bool has_next = t_next < NT;
        if constexpr (SHARED) {
            const bool next_anchor = it + 1 >= NTG;
            t_next = (next_anchor ? it + 1 - NTG : it + 1) * KVS + grp;
            seg_next = next_anchor ? seg_rows : 0;
            has_next = it + 1 < NIT && t_next < NT;
            if (blend && it == NTG) snapshot(it);
        }
        const f16* sK = smem + cur * STAGE;
        const f16* sV = sK + KT * KSTR;
        if (t >= NT) { // (KVS > 1: a ragged last round; SHARED: of either segment, and the group's next tile is not staged yet)
            if constexpr (SHARED) {
                if (has_next) {
                    load_tile(t_next, seg_next);
                    store_tile(cur ^ 1);
                }
            }
            __syncthreads();
            continue;
        }
        // ---- fragments of the tile first: K for S^T = K . Q^T and (transposed) V for O^T += V^T . P^T are read ONCE and kept
        // in registers for both query tiles; the V reads are issued here so that they land during the softmax
        // (D = 160 would need 160 registers for them and drop to one wave per SIMD: it reads at the point of use)
        f16x8 kf[HOLD ? KSTEPS : 1][4];
        f16x8 vfr[HOLD ? 2 : 1][HOLD ? NDT : 1];
        read_k(sK, kf);
        read_v(sV, vfr);
        // ---- S^T = K . Q^T, query tile by query tile: the softmax of tile a starts (VALU) while the matrix pipe is still
        // busy with tile a + 1, and further down the PV product of tile a runs under the softmax of tile a + 1
        f32x4 s[QT][4];
        qk(sK, kf, s);
        // the next tile's K/V are requested HERE, behind the fragment reads and the QK^T issue: requested at the top of the
        // iteration, the compiler's wait-count pass (it cannot count loads under divergent predicates) put a vmcnt(0) in front
        // of the first MFMA, i.e. the full global-load latency on the critical path of every tile
        if (has_next && !(abl & 1)) load_tile(t_next, seg_next);
        static_for<QT>([&](auto a_c) { softmax_pv(a_c, t, thr, s[decltype(a_c)::value], vfr, sV); });
        // (opaque to the compiler: a threshold it can see change after the first iteration makes it peel that iteration,
        // and the peeled copy costs d = 80 its register budget -- spills)
        thr = __builtin_bit_cast(int, THR);
        asm volatile("" : "+s"(thr));
        if (has_next) store_tile(cur ^ 1);
        __syncthreads();
    }

    if constexpr (KVS > 1) {
        // merge the groups' partial softmaxes: group g > 0 parks (m, l, O) of its lanes in LDS ([value][thread]: conflict-free),
        // group 0 folds them in -- the usual online-softmax combination, once -- and stores
        static_assert(KVS == 2, "the merge below handles two groups");
        float* mrg = reinterpret_cast<float*>(smem_raw);
        constexpr int NV = QT * (2 + NDT * 4);
        static_assert((size_t)NV * 256 * sizeof(float) <= (size_t)KVS * 2 * STAGE * sizeof(f16), "merge buffer fits the staging LDS");
        if (grp == 1) {
#pragma unroll
            for (int a = 0; a < QT; ++a) {
                mrg[(a * (2 + NDT * 4) + 0) * 256 + tid] = m_run[a];
                mrg[(a * (2 + NDT * 4) + 1) * 256 + tid] = l_run[a];
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) mrg[(a * (2 + NDT * 4) + 2 + dt * 4 + r) * 256 + tid] = o[a][dt][r];
            }
        }
        __syncthreads();
        if (grp == 1) return;
#pragma unroll
        for (int a = 0; a < QT; ++a) {
            const float m1 = mrg[(a * (2 + NDT * 4) + 0) * 256 + tid], l1 = mrg[(a * (2 + NDT * 4) + 1) * 256 + tid];
            const float m = fmaxf(m_run[a], m1);
            const float a0 = __builtin_amdgcn_exp2f(m_run[a] - m), a1 = __builtin_amdgcn_exp2f(m1 - m);
            // (the fused multiply-add is spelled out: which of the two products the compiler contracts is otherwise its choice per
            // instantiation, and the SHARED kernel must return the plain one's bits where it walks one segment)
            l_run[a] = __builtin_fmaf(l_run[a], a0, l1 * a1);
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    o[a][dt][r] = __builtin_fmaf(o[a][dt][r], a0, mrg[(a * (2 + NDT * 4) + 2 + dt * 4 + r) * 256 + tid] * a1);
            m_run[a] = m;
        }
    }
    // ---- normalise and store: lane holds O[q = qrow][dv = dt*16 + 4g + r]
#pragma unroll
    for (int a = 0; a < QT; ++a) {
        float l;
        if (SUM_BY_MFMA) {
            // the row sum sits in output column D = (D / 16) * 16 + 4 g + r  ->  lane group g = (D % 16) / 4, register r = D % 4
            l = __shfl(o[a][D / 16][D % 4], ((D % 16) / 4) * 16 + li);
        } else {
            l = quad_rows_sum(l_run[a]);
        }
        const float inv = l > 0.f ? 1.0f / l : 0.f;
        if (qrow[a] < p.Lq) {
            f16* op;
            if constexpr (TILED) op = p.out + (row0 + tile_row(p, qrow[a])) * p.ldo + h * D;
            else op = p.out + ((size_t)b * p.Lq + qrow[a]) * p.ldo + h * D;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                const int dv0 = dt * 16 + g * 4;
                if (dv0 < D) {
                    f16x4 hv;
                    if (SHARED && blend) { // w * softmax(own) V, parked here by snapshot(), + (1 - w) * softmax(both) V
                        const f16x4 own = *reinterpret_cast<const f16x4*>(op + dv0);
                        const float rest = (1.f - self_w) * inv;
#pragma unroll
                        for (int r = 0; r < 4; ++r) hv[r] = (f16)((float)own[r] + o[a][dt][r] * rest);
                    } else if constexpr (SHARED && KVS > 1) {
                        // the plain split kernel rounds the product to fp32 and then to fp16; beside the blend branch the compiler
                        // would fuse some of these into one mixed-precision instruction with ONE rounding, a last-bit difference in
                        // about one element in 40000.  The product goes through an opaque statement so that both round twice.
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float prod = o[a][dt][r] * inv;
                            asm volatile("" : "+v"(prod));
                            hv[r] = (f16)prod;
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) hv[r] = (f16)(o[a][dt][r] * inv);
                    }
                    *reinterpret_cast<f16x4*>(op + dv0) = hv;
                }
            }
        }
    }
}


// The operand rules both entry points share (a macro so that the message names the entry point): head dim, strides, alignment, scale.
// d = 64 / 160 take the row maximum on the RAW scores and scale it afterwards, which is the maximum of the scaled scores
// only for scale > 0; no caller passes anything else
#define SDOD_ATTN_REQUIRE_OPERANDS(q, k, v, out, heads, d, ldq, ldk, ldv, ldo, scale)                                                   \
    do {                                                                                                                               \
        SDOD_REQUIRE(sdod_attention_head_dim_ok(d), "head dim must be one of 40, 64, 80, 160");                                        \
        SDOD_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 4 == 0, "row strides must keep 16-byte alignment");         \
        SDOD_REQUIRE(ldq >= heads * d && ldk >= heads * d && ldv >= heads * d && ldo >= heads * d, "row stride < heads*d");            \
        SDOD_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) == 0 && ((uintptr_t)out & 7) == 0, "misaligned pointer");     \
        SDOD_REQUIRE(std::isfinite(scale) && scale > 0.f, "scale must be finite and > 0");                                             \
    } while (0)

// P is AttnP, AttnTP or AttnSP, and with it the kernel's TILED / SHARED parameters
template <int D, int QT, bool TR, int KVS = 1, class P>
hipError_t attn_launch(const P& p, hipStream_t st) {
    constexpr bool TILED = std::is_same_v<P, AttnTP>, SHARED = std::is_same_v<P, AttnSP>;
    constexpr int DP = ((D + 31) / 32) * 32;
    constexpr int DV = ((D + 15) / 16) * 16;
    constexpr size_t smem = (size_t)KVS * 2 * 64 * (DP + 8 + odd16(DV)) * sizeof(f16);
    static_assert(smem <= 160 * 1024, "LDS");
    static std::atomic<unsigned long long> attr_devs{0};
    if (sdod::first_use_on_device(attr_devs)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_kernel<D, QT, TR, KVS, TILED, SHARED>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return e;
    }
    dim3 grid(((p.Lq + 64 * QT - 1) / (64 * QT)) * p.H * p.B);
    SDOD_LAUNCH((attn_kernel<D, QT, TR, KVS, TILED, SHARED>), grid, dim3(256 * KVS), smem, st, p);
    return hipGetLastError();
}

template <int D, class P>
hipError_t attn_dispatch(const P& p, bool big, bool tr, hipStream_t st) {
    if (tr) return big ? attn_launch<D, 2, true>(p, st) : attn_launch<D, 1, true>(p, st);
    return big ? attn_launch<D, 2, false>(p, st) : attn_launch<D, 1, false>(p, st);
}

// The ONE choice of kernel form, from the head dim and p's B / H / Lq / Lk / causal: query tiles per wave, the d = 80 key/value split,
// the developer overrides.  sdod_attention_tiled_f16 comes here with B = (image, tile) pairs and Lq = Lk = th * tw, so a tile runs
// the form -- and the arithmetic, bit for bit -- that sdod_attention_f16 runs on the tile's rows gathered into a tensor of their own.
template <class P>
hipError_t attn_run(const P& p, int d, hipStream_t st) {
    const bool no_tr = std::getenv("SDOD_ATTN_NO_TR") != nullptr; // debugging aid: scalar LDS reads instead of ds_read_b64_tr_b16
    const bool tr = !no_tr;
    bool big = p.Lq >= 2048 && d != 160; // two query tiles per wave once there is enough work to fill the chip
    // developer override (tools/attn_bench.py), read on EVERY call: tests/test_attention_paths_gpu.py relies on that to run the
    // two-query-tile kernels (SDOD_ATTN_QT=2) at small shapes and the one-tile kernels (=1) on the same data
    if (const char* e = std::getenv("SDOD_ATTN_QT")) big = e[0] == '2' && d != 160;
    switch (d) {
    case 40: return attn_dispatch<40>(p, big, tr, st);
    case 64: return attn_dispatch<64>(p, big, tr, st);
    case 80: {
        // one workgroup per CU or less and at least four key tiles: split the keys inside the workgroup (two groups of four waves)
        // (19.4 vs 21.3 us at 32x32, tools/attn_bench.py; SDOD_ATTN_KVS=0 keeps the four-wave form)
        static const bool kvs_off = [] { const char* e2 = std::getenv("SDOD_ATTN_KVS"); return e2 && e2[0] == '0'; }();
        const long long wgs = (long long)((p.Lq + 63) / 64) * p.H * p.B;
        if (!big && tr && !kvs_off && !p.causal && wgs <= 512 && p.Lk >= 256) return attn_launch<80, 1, true, 2>(p, st);
        return attn_dispatch<80>(p, big, tr, st);
    }
    default: return attn_dispatch<160>(p, false, tr, st);
    }
}
} // namespace
