// attention.hip -- fused softmax(scale * Q K^T) V for the UNet's self/cross attention and CLIP's causal
// attention on gfx950.  In the reference these are the `/attn*/to_*`, `/smax/`, `/MatMul` ops inside the
// opaque UNet / text-encoder QNN graphs (analyze_results.py:69-79; executed at qnn_context.cpp:711-713).
//
// The score matrix (4096x4096 per head-batch at the 64x64 level) never touches HBM: a workgroup owns
// 64*QT query rows of one (batch, head), walks K/V in 64-key tiles staged through LDS (register
// prefetch, double-buffered, one barrier per tile) and keeps an online softmax in registers.
//
// wave64 / MFMA mapping (v_mfma_f32_16x16x32_f16), chosen so that NO cross-lane data movement is needed
// between the two matrix products:
//   * S^T = K . Q^T  (K rows are the MFMA "A" operand, Q rows the "B" operand): lane l ends up with the
//     scores of ONE query (column l&15) against keys 16*t + 4*(l>>4) + r  -> the row max / row sum are
//     in-lane reductions plus two xor-shuffles (16, 32);
//   * O^T = V^T . P^T: the P registers a lane already holds ARE its B-operand fragment (keys on the
//     contraction axis), and V^T fragments come from the row-major V tile through the gfx950
//     transposed LDS read ds_read_b64_tr_b16 (4 keys x 16 columns per 16-lane group);
//   * O^T keeps the query on the lane, so the online-softmax rescale is a per-lane scalar multiply.
// Head dims 40/80/160 (SD v1) and 64 (CLIP, SD v2) are zero-padded in LDS to the MFMA granularity.
#include "attention_kernel.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Folded cross-attention (once per prompt).  The text context -- and with it every cross-attention K and V -- is constant
// over the sampler run, so the two Linears around the attention can be multiplied INTO K and V:
//   scores_h = LN(x) Wq_h^T K_h^T = LN(x) . W1_h,      W1_h = Wq_h^T K_h^T   [C x L]
//   out      = sum_h P_h V_h Wo_h^T = [P_1 | ... | P_H] . [W2_1 ; ... ; W2_H],   W2_h = V_h Wo_h^T   [L x C]
// i.e. per evaluation the block is TWO plain GEMMs (the softmax runs in the epilogue of the first, sdod_gemm_desc::softmax_cols)
// instead of Linear + attention kernel + Linear; L = 77 keys are padded to 80 columns per head.  This kernel builds the
// per-image matrices: C[bt][m][n] = alpha * sum_k A[bt][m][k] B[bt][n][k] for many small (64 x 64 x d) problems with arbitrary
// element strides (the operands are slices of the K|V projection and of the weight matrices), rows / columns past the valid
// range produce zeros.  fp16 in, fp32 accumulate, fp16 out; 16 outputs per thread from LDS tiles.
struct FoldP {
    const f16* kv; int ld_kv, k_off, v_off, L, n_img;
    const f16* wq; int ldq;
    const float* sq; const float* tq;
    const f16* wo; int ldwo;
    int heads, d, C;
    float alpha;
    f16* w1; float* s1; float* t1; f16* w2;
    int tiles_c; // C / 80
    int n_w;     // work items of W1 (and of W2): n_img * heads * tiles_c
    int regions; // sdod_xattn_fold_regions_f16: n_img counts (image, region) segments; W2 puts a segment's columns behind its image's
                 // earlier regions, [C][regions * NK].  1 = one segment per image
    // sdod_xattn_fold_ip_f16 (regions == 2): the odd segments come from a second K/V source with a length and strides of its own
    const f16* kv2; int ld_kv2, k_off2, v_off2, L2; // kv2 == nullptr: every segment from kv
};
constexpr int kFoldKMax = 160;
// where segment `seg` of n_img finds its keys and values: rows [0, L) at k / v, row stride ld.  TWO_SRC is a compile-time switch so
// that the one-source kernel, which every plain graph runs 16 times per prompt, carries no test of kv2 and no pointer selects
struct FoldSeg { const f16* k; const f16* v; int ld, L; };
template <bool TWO_SRC>
__device__ __forceinline__ FoldSeg fold_segment(const FoldP& p, int seg) {
    if constexpr (!TWO_SRC) {
        const f16* base = p.kv + (long long)seg * p.L * p.ld_kv;
        return FoldSeg{base + p.k_off, base + p.v_off, p.ld_kv, p.L};
    }
    const int b = seg >> 1; // segment 2 b = image b's text keys, 2 b + 1 = its image tokens
    if (seg & 1) {
        const f16* base = p.kv2 + (long long)b * p.L2 * p.ld_kv2;
        return FoldSeg{base + p.k_off2, base + p.v_off2, p.ld_kv2, p.L2};
    }
    const f16* base = p.kv + (long long)b * p.L * p.ld_kv;
    return FoldSeg{base + p.k_off, base + p.v_off, p.ld_kv, p.L};
}
// One launch per transformer block: workgroups [0, n_w) build 80 x 80 tiles of W1 (rows = a head's 80 key slots, columns = 80
// input channels), [n_w, 2 n_w) tiles of W2 (rows = 80 output channels, columns = a head's key slots), the rest the fold
// vectors.  Both products contract over the head dimension d (<= 160, zero-padded to the MFMA's 32): operands staged in LDS as
// [row][k], v_mfma_f32_16x16x32_f16, 5 x 5 blocks of 16 x 16 per tile over 4 waves.
template <bool TWO_SRC>
__global__ __launch_bounds__(256) void xattn_fold_kernel(const FoldP p) {
    __shared__ __attribute__((aligned(16))) f16 sa[80][kFoldKMax + 8], sb[80][kFoldKMax + 8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NK = p.heads * 80, d = p.d;
    int item = blockIdx.x;
    if (item >= 2 * p.n_w) {
        // fold vectors of the score GEMM: s1 = alpha * K_h . s_q, t1 = alpha * K_h . t_q; padding columns: s = 0 and a bias that
        // the softmax turns into an exact zero
        const int idx = (item - 2 * p.n_w) * 256 + tid;
        if (idx >= p.n_img * NK) return;
        const int j = idx % 80, bh = idx / 80, h = bh % p.heads, img = bh / p.heads;
        const FoldSeg sg = fold_segment<TWO_SRC>(p, img);
        if (j >= sg.L) {
            p.s1[idx] = 0.f;
            p.t1[idx] = -30000.f;
            return;
        }
        const f16* kr = sg.k + (long long)j * sg.ld + h * d;
        float a = 0.f, b = 0.f;
        for (int dd = 0; dd < d; ++dd) {
            const float kval = (float)kr[dd];
            a = fmaf(kval, p.sq[h * d + dd], a);
            b = fmaf(kval, p.tq[h * d + dd], b);
        }
        p.s1[idx] = p.alpha * a;
        p.t1[idx] = p.alpha * b;
        return;
    }
    const bool second = item >= p.n_w;
    if (second) item -= p.n_w;
    const int tc = item % p.tiles_c, bh = item / p.tiles_c, h = bh % p.heads, img = bh / p.heads;
    const int KP = (d + 31) & ~31, kc = KP / 8;
    const FoldSeg sg = fold_segment<TWO_SRC>(p, img);
    // rows of K / V (key slots; slots past L and columns past d are zero) and of Wo: contiguous along k, 16-byte pieces
    auto stage_rows = [&](f16 (*dst)[kFoldKMax + 8], const f16* base, long long row_stride, int valid_rows) {
        for (int idx = tid; idx < 80 * kc; idx += 256) {
            const int r = idx / kc, ch = idx - r * kc;
            const f16x8 v = (r < valid_rows && ch * 8 < d) ? ldg8(base + (long long)r * row_stride + ch * 8) : zero8();
            *reinterpret_cast<f16x8*>(&dst[r][ch * 8]) = v;
        }
    };
    if (!second) {
        stage_rows(sa, sg.k + h * d, sg.ld, sg.L);
        // Wq'[(h, k)][c]: contiguous along c -> transposed into [c][k]
        for (int idx = tid; idx < KP * 10; idx += 256) {
            const int k = idx / 10, ch = idx - k * 10;
            const f16x8 v = k < d ? ldg8(p.wq + (long long)(h * d + k) * p.ldq + tc * 80 + ch * 8) : zero8();
#pragma unroll
            for (int e = 0; e < 8; ++e) sb[ch * 8 + e][k] = v[e];
        }
    } else {
        stage_rows(sa, p.wo + (long long)(tc * 80) * p.ldwo + h * d, p.ldwo, 80);
        stage_rows(sb, sg.v + h * d, sg.ld, sg.L);
    }
    __syncthreads();
    const int fr = lane & 15, fg = lane >> 4;
    for (int rb = wave; rb < 5; rb += 4) { // (wave-uniform)
        f32x4 acc[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < KP / 32; ++ks) {
            const f16x8 fa = *reinterpret_cast<const f16x8*>(&sa[rb * 16 + fr][ks * 32 + fg * 8]);
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const f16x8 fb = *reinterpret_cast<const f16x8*>(&sb[j * 16 + fr][ks * 32 + fg * 8]);
                acc[j] = mfma16(fb, fa, acc[j]); // lane: row rb*16 + fr, columns j*16 + 4 fg + r
            }
        }
        const int m = rb * 16 + fr;
        const int wimg = img / p.regions, reg = img - wimg * p.regions;
        f16* row = second ? p.w2 + ((long long)wimg * p.C + tc * 80 + m) * ((long long)p.regions * NK) + reg * NK + h * 80
                          : p.w1 + ((long long)(img * p.heads + h) * 80 + m) * p.C + tc * 80;
        const float al = second ? 1.0f : p.alpha;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            f16x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = (f16)(al * acc[j][r]);
            *reinterpret_cast<f16x4*>(row + j * 16 + fg * 4) = o;
        }
    }
}

} // namespace

// the head dims the fused attention kernel is instantiated for (the `switch (d)` below): the ONE list.  Host-only.
extern "C" int sdod_attention_head_dim_ok(int d) { return d == 40 || d == 64 || d == 80 || d == 160 ? 1 : 0; }

// the folded cross-attention's contract (include/sdod_hip.h).  Host-only.
extern "C" int sdod_xattn_fold_ok(int heads, int d, int l_keys, int rows_per_image) {
    // the fold launch: d zero-padded to the MFMA's 32 within kFoldKMax columns of LDS and read in 16-byte pieces; 80 key slots per
    // head; W1 / W2 are written as 80-channel tiles (tiles_c = heads * d / 80)
    if (heads <= 0 || d <= 0 || d > kFoldKMax || d % 8 != 0 || l_keys <= 0 || l_keys > 80) return 0;
    const long long C = (long long)heads * d, NK = (long long)heads * 80;
    if (C % 80 != 0) return 0;
    if (rows_per_image == 0) return 1;
    // the two GEMMs of every evaluation: K = heads * d of the score GEMM and K = heads * 80 of the second one in 64-deep slabs
    // (the latter also makes N = heads * 80 of the score GEMM a multiple of 160: whole softmax groups per tile), per-image
    // weights on tiles of at least 32 rows
    return rows_per_image > 0 && rows_per_image % 32 == 0 && NK % 320 == 0 && C % 64 == 0 ? 1 : 0;
}

extern "C" int sdod_attention_f16(const void* q, const void* k, const void* v, void* out, int batch, int heads, int lq,
                                  int lk, int d, int ldq, int ldk, int ldv, int ldo, float scale, int causal,
                                  void* stream) {
    SDOD_TRY
    SDOD_REQUIRE(q && k && v && out, "null pointer");
    SDOD_REQUIRE(batch > 0 && heads > 0 && lq > 0 && lk > 0, "bad shape");
    SDOD_ATTN_REQUIRE_OPERANDS(q, k, v, out, heads, d, ldq, ldk, ldv, ldo, scale);
    AttnP p{};
    p.q = (const f16*)q; p.k = (const f16*)k; p.v = (const f16*)v; p.out = (f16*)out;
    p.B = batch; p.H = heads; p.Lq = lq; p.Lk = lk;
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
    p.scale_log2 = scale * 1.4426950408889634f;
    p.causal = causal;
    SDOD_HIP_CHECK(attn_run(p, d, (hipStream_t)stream));
    return 0;
    SDOD_CATCH
}

namespace {
// the image-token source of sdod_xattn_fold_ip_f16; kv == nullptr for the one-source calls
struct FoldSrc2 { const void* kv; int ld, k_off, v_off, L; };
int xattn_fold_launch(const void* kv, int ld_kv, int k_off, int v_off, int n_img, int regions, int L, const void* wq, int ldq, const void* sq,
                      const void* tq, const void* wo, int ldwo, int heads, int d, float scale, void* w1, void* s1, void* t1, void* w2,
                      void* stream, const FoldSrc2& ip = FoldSrc2{nullptr, 0, 0, 0, 0}) {
    SDOD_TRY
    SDOD_REQUIRE(regions >= 1 && regions <= 4, "regions must be in [1, 4]");
    if (ip.kv) {
        SDOD_REQUIRE(regions == 2, "two sources are two segments per image");
        SDOD_REQUIRE(ip.L >= 1 && ip.L <= 16, "image tokens must be in [1, 16]");
        SDOD_REQUIRE(ip.ld % 8 == 0 && ip.k_off % 8 == 0 && ip.v_off % 8 == 0 && ip.k_off >= 0 && ip.v_off >= 0 && ((uintptr_t)ip.kv & 15) == 0,
                     "operands must keep 16-byte alignment");
        SDOD_REQUIRE(heads > 0 && d > 0 && (long long)ip.k_off + (long long)heads * d <= ip.ld && (long long)ip.v_off + (long long)heads * d <= ip.ld,
                     "image K / V offsets + heads * d must fit the image row stride");
    }
    SDOD_REQUIRE(n_img <= (1 << 20), "bad shape (too many images)");
    n_img *= regions; // (image, region) segments of L rows
    SDOD_REQUIRE(kv && wq && sq && tq && wo && w1 && s1 && t1 && w2, "null pointer");
    // (rows_per_image 0: the launch's own part of the contract; the builder asks with the rows of its two GEMMs)
    SDOD_REQUIRE(n_img > 0 && sdod_xattn_fold_ok(heads, d, L, 0), "bad shape (d <= 160, d % 8 == 0, L <= 80, heads * d a multiple of 80)");
    SDOD_REQUIRE((long long)heads * d <= (1 << 24), "bad shape (heads * d too large)");
    const int C = heads * d, NK = heads * 80;
    SDOD_REQUIRE(ldq >= C && ldwo >= C && ld_kv >= C, "row strides >= heads * d");
    SDOD_REQUIRE(ld_kv % 8 == 0 && k_off % 8 == 0 && v_off % 8 == 0 && ldq % 8 == 0 && ldwo % 8 == 0 &&
                     (((uintptr_t)kv | (uintptr_t)wq | (uintptr_t)wo | (uintptr_t)w1 | (uintptr_t)w2) & 15) == 0,
                 "operands must keep 16-byte alignment");
    FoldP p{};
    p.kv = (const f16*)kv; p.ld_kv = ld_kv; p.k_off = k_off; p.v_off = v_off; p.L = L; p.n_img = n_img;
    p.wq = (const f16*)wq; p.ldq = ldq; p.sq = (const float*)sq; p.tq = (const float*)tq;
    p.wo = (const f16*)wo; p.ldwo = ldwo;
    p.heads = heads; p.d = d; p.C = C;
    p.alpha = scale * 1.4426950408889634f; // the softmax of the score GEMM's epilogue works in the exp2 domain
    p.w1 = (f16*)w1; p.s1 = (float*)s1; p.t1 = (float*)t1; p.w2 = (f16*)w2;
    p.tiles_c = C / 80;
    p.n_w = n_img * heads * p.tiles_c;
    p.regions = regions;
    p.kv2 = (const f16*)ip.kv; p.ld_kv2 = ip.ld; p.k_off2 = ip.k_off; p.v_off2 = ip.v_off; p.L2 = ip.L;
    const int blocks = 2 * p.n_w + (n_img * NK + 255) / 256;
    if (ip.kv) SDOD_LAUNCH(xattn_fold_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
    else SDOD_LAUNCH(xattn_fold_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
    SDOD_HIP_CHECK(hipGetLastError());
    return 0;
    SDOD_CATCH
}
} // namespace

extern "C" int sdod_xattn_fold_f16(const void* kv, int ld_kv, int k_off, int v_off, int n_img, int L, const void* wq, int ldq,
                                   const void* sq, const void* tq, const void* wo, int ldwo, int heads, int d, float scale, void* w1,
                                   void* s1, void* t1, void* w2, void* stream) {
    return xattn_fold_launch(kv, ld_kv, k_off, v_off, n_img, 1, L, wq, ldq, sq, tq, wo, ldwo, heads, d, scale, w1, s1, t1, w2, stream);
}

extern "C" int sdod_xattn_fold_regions_f16(const void* kv, int ld_kv, int k_off, int v_off, int n_img, int regions, int L, const void* wq,
                                           int ldq, const void* sq, const void* tq, const void* wo, int ldwo, int heads, int d, float scale,
                                           void* w1, void* s1, void* t1, void* w2, void* stream) {
    return xattn_fold_launch(kv, ld_kv, k_off, v_off, n_img, regions, L, wq, ldq, sq, tq, wo, ldwo, heads, d, scale, w1, s1, t1, w2, stream);
}

extern "C" int sdod_xattn_fold_ip_f16(const void* kv, int ld_kv, int k_off, int v_off, const void* kv_ip, int ld_ip, int k_off_ip, int v_off_ip,
                                      int n_img, int L, int T, const void* wq, int ldq, const void* sq, const void* tq, const void* wo, int ldwo,
                                      int heads, int d, float scale, void* w1, void* s1, void* t1, void* w2, void* stream) {
    SDOD_TRY
    SDOD_REQUIRE(kv_ip, "null pointer");
    SDOD_CATCH
    return xattn_fold_launch(kv, ld_kv, k_off, v_off, n_img, 2, L, wq, ldq, sq, tq, wo, ldwo, heads, d, scale, w1, s1, t1, w2, stream,
                             FoldSrc2{kv_ip, ld_ip, k_off_ip, v_off_ip, T});
}
