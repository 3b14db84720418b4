// graphs.hip -- launch-list builders, one per graph kind (include/sdod_engine.h): UNet eps-model (with the inpainting, T2I-Adapter
// and seamless-tiling variants of its inputs), time-embedding MLP, CLIP text encoder, VAE decoder, VAE encoder and its masked form
// (img2img, inpainting), T2I-Adapter, ESRGAN upscaler, ControlNet and its hint encoder, CLIP image encoder and IP-Adapter image
// projection.  The first four stand in for the serialized QNN graphs the reference loads
// (context.cpp:105: "unet.serialized", "text_encoder.serialized", "vae_decoder.serialized", "temb"); the
// block structure follows the op names visible in the reference's own profiler table
// (analyze_results.py:20-93: in_layers / emb_layers / out_layers / skip_connection, norm / proj_in /
// transformer_blocks.0.{norm1-3, attn1, attn2, ff.net.0.proj, ff.net.2} / proj_out) and the public SD v1.x
// architecture.  Parameter names are the CompVis-ldm / HF-CLIP state-dict keys.
//
// Fusions decided here (all are reads/writes removed from HBM, the UNet sits at the roofline ridge):
//   * SiLU into every ResBlock GroupNorm; the skip-connection channel concat into the GroupNorm reads and
//     into the conv gathers (no concat tensor); nearest-2x upsampling into the conv gather;
//   * conv bias + time-embedding broadcast + residual into the conv epilogue;
//   * to_q/to_k/to_v as ONE GEMM (weights contiguous in the arena); all 22 ResBlock time-embedding
//     projections as ONE GEMM per UNet evaluation; attention output / FF output residuals in the GEMM epilogue;
//   * z/0.18215 and post_quant_conv into the latent layout change.
#include "engine.h"

namespace sdod {

// channel multiplier per resolution level: UNet and T2I-Adapter on model_channels, both VAE halves on vae_channels
static const int kChMult[4] = {1, 2, 4, 4};

int Graph::group_first(const std::string& group) const {
    auto it = gindex_.find(group);
    if (it == gindex_.end()) throw Error(INTERNAL_ERROR, "unknown parameter group " + group);
    return groups_[it->second].front();
}

const char* Graph::group_base(const std::string& group) const {
    auto it = gindex_.find(group);
    if (it == gindex_.end()) throw Error(INTERNAL_ERROR, "unknown parameter group " + group);
    return params_[groups_[it->second].front()].dev;
}

// ------------------------------------------------------------------------------------------------ UNet
Act Graph::res_block(const std::string& pfx, const Act& x, const Act* x2, int cout, const f16* emb_all, int emb_ld, int& emb_off) {
    const int cin = x.c + (x2 ? x2->c : 0);
    quant_rows(x.rows());
    const int n1w = P(pfx + ".in_layers.0.weight", {cin}, PK_VEC), n1b = P(pfx + ".in_layers.0.bias", {cin}, PK_VEC);
    const int c1w = P(pfx + ".in_layers.2.weight", {cout, cin, 3, 3}, PK_CONV3), c1b = P(pfx + ".in_layers.2.bias", {cout}, PK_VEC);
    const int n2w = P(pfx + ".out_layers.0.weight", {cout}, PK_VEC), n2b = P(pfx + ".out_layers.0.bias", {cout}, PK_VEC);
    // out_layers.3 (3x3) and skip_connection (1x1) share ONE weight matrix [cout][9*cout + cin]: the skip conv is the tail
    // K-segment of the same GEMM (one launch, no intermediate skip tensor)
    int c2w, skw = -1, skb = -1;
    const bool fuse_skip = !quant_decl_; // uint8 weights: the skip conv's tensor has its own encoding -> its own GEMM
    if (cin != cout && !fuse_skip) {
        c2w = P(pfx + ".out_layers.3.weight", {cout, cout, 3, 3}, PK_CONV3);
        skw = P(pfx + ".skip_connection.weight", {cout, cin, 1, 1}, PK_CONV1);
        skb = P(pfx + ".skip_connection.bias", {cout}, PK_VEC);
    } else if (cin != cout) {
        const int ld = 9 * cout + cin;
        c2w = Pc(pfx + ".out_layers.3.weight", {cout, cout, 3, 3}, PK_CONV3, ld, 0, -1);
        skw = Pc(pfx + ".skip_connection.weight", {cout, cin, 1, 1}, PK_CONV1, ld, 9 * cout, c2w);
        skb = P(pfx + ".skip_connection.bias", {cout}, PK_VEC);
    } else {
        c2w = P(pfx + ".out_layers.3.weight", {cout, cout, 3, 3}, PK_CONV3);
    }
    const int c2b = P(pfx + ".out_layers.3.bias", {cout}, PK_VEC);
    (void)skw;
    const int my_off = emb_off;
    emb_off += cout;

    Act g1 = group_norm(x, x2, n1w, n1b, 1e-5f, true);
    GemmOpt o1;
    o1.bias = c1b;
    o1.row_bias = emb_all ? emb_all + my_off : nullptr;
    o1.ld_row_bias = emb_ld;
    o1.rows_per_img = x.h * x.w;
    Act h = conv(g1, nullptr, c1w, cout, 3, 1, false, o1);
    release(g1);
    Act g2 = group_norm(h, nullptr, n2w, n2b, 1e-5f, true);
    release(h);
    GemmOpt o2;
    o2.bias = c2b;
    Act sk;
    if (cin != cout && !fuse_skip) {
        GemmOpt os;
        os.bias = skb;
        sk = conv(x, x2, skw, cout, 1, 1, false, os); // 1x1 over the (possibly concatenated) block input
        o2.residual = sk.p;
    } else if (cin != cout) {
        o2.tail0 = &x;
        o2.tail1 = x2;
        o2.bias2 = skb;
    } else {
        if (x2) throw Error(INTERNAL_ERROR, "identity skip with a concatenated input");
        o2.residual = x.p;
    }
    Act out = conv(g2, nullptr, c2w, cout, 3, 1, false, o2);
    release(g2);
    if (sk.p) release_after_consumer(sk);
    return out;
}

Graph::HeadGeom Graph::head_geometry(int C) const {
    const int nh = cfg_.num_heads, hd = cfg_.head_dim;
    const std::string at = " (transformer on " + std::to_string(C) + " channels)";
    SDOD_REQUIRE(nh >= 0, "num_heads must not be negative (0 = head_dim decides)");
    HeadGeom g;
    if (nh > 0) { // num_heads decides, head_dim is ignored
        SDOD_REQUIRE(C % nh == 0, "num_heads must divide the channels of every transformer" + at);
        g.heads = nh;
        g.d = C / nh;
        SDOD_REQUIRE(sdod_attention_head_dim_ok(g.d), "num_heads gives head dim " + std::to_string(g.d) + ", which no attention kernel takes (40, 64, 80, 160)" + at);
    } else {
        SDOD_REQUIRE(hd > 0, "head_dim must be positive when num_heads is 0 (one of num_heads / head_dim decides the head geometry)");
        SDOD_REQUIRE(C % hd == 0, "head_dim must divide the channels of every transformer" + at);
        SDOD_REQUIRE(sdod_attention_head_dim_ok(hd), "head_dim must be one the attention kernel takes (40, 64, 80, 160)");
        g.heads = C / hd;
        g.d = hd;
    }
    return g;
}

void Graph::check_head_geometry() const {
    for (int m : {1, 2, 4}) (void)head_geometry(m * cfg_.model_channels);
}

Act Graph::spatial_transformer(const std::string& pfx, const Act& x, const Act& ctx) {
    const int C = x.c, cd = ctx.c;
    const HeadGeom hg = head_geometry(C);
    const int heads = hg.heads, d = hg.d;
    const int rows = x.rows(), L = x.h * x.w, B = x.n;
    const std::string tb = pfx + ".transformer_blocks.0";
    quant_rows(rows);
    const bool quant_block = quant_decl_;
    const int nw = P(pfx + ".norm.weight", {C}, PK_VEC), nb = P(pfx + ".norm.bias", {C}, PK_VEC);
    const bool lin = cfg_.linear_proj != 0; // SD2.x stores these as Linear [C, C]; the arithmetic is the same
    const int piw = lin ? P(pfx + ".proj_in.weight", {C, C}, PK_LINEAR) : P(pfx + ".proj_in.weight", {C, C, 1, 1}, PK_CONV1);
    const int pib = P(pfx + ".proj_in.bias", {C}, PK_VEC);
    const int l1w = P(tb + ".norm1.weight", {C}, PK_VEC), l1b = P(tb + ".norm1.bias", {C}, PK_VEC);
    const std::string gq = tb + ".attn1.qkv";
    P(tb + ".attn1.to_q.weight", {C, C}, PK_LINEAR, gq);
    P(tb + ".attn1.to_k.weight", {C, C}, PK_LINEAR, gq);
    P(tb + ".attn1.to_v.weight", {C, C}, PK_LINEAR, gq);
    const int o1w = P(tb + ".attn1.to_out.0.weight", {C, C}, PK_LINEAR), o1b = P(tb + ".attn1.to_out.0.bias", {C}, PK_VEC);
    const int l2w = P(tb + ".norm2.weight", {C}, PK_VEC), l2b = P(tb + ".norm2.bias", {C}, PK_VEC);
    const int q2w = P(tb + ".attn2.to_q.weight", {C, C}, PK_LINEAR);
    // every layer's to_k|to_v lives in ONE group: the context projections of all 16 transformers are a single GEMM that
    // runs once per prompt (the context is constant over the sampler run), see build_unet()
    quant_global(); // (one encoding policy for the whole group: its GEMM runs on M = 77 rows per prompt)
    P(tb + ".attn2.to_k.weight", {C, cd}, PK_LINEAR, "attn2_kv_all");
    P(tb + ".attn2.to_v.weight", {C, cd}, PK_LINEAR, "attn2_kv_all");
    if (ip_tokens_ > 0) { // image prompt: the image tokens' projections, one group and one static GEMM like the text's (ip_kv_all_gemm)
        P(tb + ".attn2.to_k_ip.weight", {C, cd}, PK_LINEAR, "attn2_kv_ip_all");
        P(tb + ".attn2.to_v_ip.weight", {C, cd}, PK_LINEAR, "attn2_kv_ip_all");
    }
    quant_decl_ = quant_block;
    const int my_kv = kv_off_;
    kv_off_ += 2 * C;
    const int o2w = P(tb + ".attn2.to_out.0.weight", {C, C}, PK_LINEAR), o2b = P(tb + ".attn2.to_out.0.bias", {C}, PK_VEC);
    const int l3w = P(tb + ".norm3.weight", {C}, PK_VEC), l3b = P(tb + ".norm3.bias", {C}, PK_VEC);
    const int f1w = P(tb + ".ff.net.0.proj.weight", {8 * C, C}, PK_LINEAR_GEGLU), f1b = P(tb + ".ff.net.0.proj.bias", {8 * C}, PK_VEC_GEGLU);
    // ff.net.2 and proj_out follow each other with nothing but a residual add in between:
    //   out = P (W2 g + b2 + t2) + bp + x = [P W2 | P] [g ; t2] + (P b2 + bp) + x
    // so the two Linears (analyze_results.py:69-79 lists them as separate ops) are ONE GEMM over K = 5C on the row-wise concat
    // [g | t2]: both weights live in one [C][5C] matrix whose first 4C columns are replaced by P W2 at finalize
    // (sdod_compose_linear_f16, fp32 accumulate, one fp16 rounding), GEGLU writes g and attn2.to_out writes t2 straight into the
    // concatenated buffer.  One launch and one [rows][C] round trip less per transformer block.  Not with uint8 weights (integer
    // codes cannot be composed); SDOD_COMPOSE=0 keeps the two-GEMM form (A/B switch).
    static const bool compose_on = [] { const char* e = std::getenv("SDOD_COMPOSE"); return !(e && e[0] == '0'); }();
    const bool compose = compose_on && !quant_block;
    int f2w, pow_;
    if (compose) {
        f2w = Pc(tb + ".ff.net.2.weight", {C, 4 * C}, PK_LINEAR, 5 * C, 0, -1);
        pow_ = lin ? Pc(pfx + ".proj_out.weight", {C, C}, PK_LINEAR, 5 * C, 4 * C, f2w)
                   : Pc(pfx + ".proj_out.weight", {C, C, 1, 1}, PK_CONV1, 5 * C, 4 * C, f2w);
    } else {
        f2w = P(tb + ".ff.net.2.weight", {C, 4 * C}, PK_LINEAR);
        pow_ = lin ? P(pfx + ".proj_out.weight", {C, C}, PK_LINEAR) : P(pfx + ".proj_out.weight", {C, C, 1, 1}, PK_CONV1);
    }
    const int f2b = P(tb + ".ff.net.2.bias", {C}, PK_VEC);
    const int pob = P(pfx + ".proj_out.bias", {C}, PK_VEC);
    if (mode_ == DECLARE) return act(x.n, x.h, x.w, C);

    // ---- 1. proj_in
    Act g = group_norm(x, nullptr, nw, nb, 1e-6f, false);
    Act t0 = act(B, 1, L, C);
    { GemmOpt o; o.bias = pib; linear(g.p, rows, C, piw, C, t0.p, o); }
    release(g);
    // the three LayerNorms of the block are folded into the Linear that consumes them (no LN launch, no LN tensor) -- except
    // with uint8 weights, whose integer codes cannot absorb gamma: there LayerNorm is a launch and the Linear a plain one.
    // gemm(a, o) emits that Linear on the rows at `a`; its output is allocated by the caller, BEFORE the normalised tensor.
    const bool fold = !quant_block;
    auto behind_ln = [&](const Act& src, int lw, int lb, GemmOpt o, auto gemm) {
        if (fold) {
            o.ln_w = lw; o.ln_b = lb;
            gemm(src.p, o);
        } else { // (uint8 weights are never composed: src is a dense [rows][C] tensor)
            Act nrm = layer_norm(src, lw, lb, 1e-5f);
            gemm(nrm.p, o);
            release(nrm);
        }
    };
    // ---- 2. self-attention
    f16* qkv = alloc((size_t)rows * 3 * C);
    { GemmOpt o; o.wq_scale = qscale_of(group_first(gq)); o.wq_off = qoff_of(group_first(gq)); // (null unless the block keeps uint8 codes)
      behind_ln(t0, l1w, l1b, o, [&](const f16* a, const GemmOpt& og) {
          linear_raw(a, rows, C, reinterpret_cast<const f16*>(group_base(gq)), C, 3 * C, qkv, og); }); }
    f16* a1 = alloc((size_t)rows * C);
    attention(qkv, qkv + C, qkv + 2 * C, a1, B, heads, L, L, d, 3 * C, 3 * C, 3 * C, C, false);
    release(qkv);
    Act t1 = act(B, 1, L, C);
    { GemmOpt o; o.bias = o1b; o.residual = t0.p; linear(a1, rows, C, o1w, C, t1.p, o); }
    release(a1); release(t0);
    // ---- 3. cross-attention on the text context, in two forms
    // FOLDED form (attention.hip: sdod_xattn_fold_f16): the context, and with it K and V,
    // is constant over the sampler run, so to_q is multiplied into K and to_out into V once per prompt (static launch list) and
    // the block is two GEMMs per evaluation -- scores = LN(t1) . (Wq^T K_h^T) with the row softmax over each head's 77 (+3
    // padding) columns in the epilogue, then [P_1 | .. | P_H] . (V_h Wo_h^T) + bias + residual -- instead of Linear + attention
    // kernel + Linear: one launch less per block, and at the deep levels half the weight bytes (2 x 640 x C against 2 x C x C).
    // Needs the LayerNorm fold (fp16 weights), heads * 80 columns tiled by the 160-wide GEMM tiles and the 64-deep K slabs,
    // image rows a multiple of 32.  SDOD_XATTN_FOLD=0 keeps the three-launch form (A/B switch).
    static const bool xfold_on = [] { const char* e = std::getenv("SDOD_XATTN_FOLD"); return !(e && e[0] == '0'); }();
    // REGIONAL PROMPTS (regions_ > 0): the context holds regions_ prompts of Lk keys per image and the block's output is
    // sum_r w_r(pixel) attn(x, K_r, V_r).  Folded: the score GEMM's 80-column groups are laid out [region][head][80], its epilogue
    // multiplies each group by its region's weight at the row's pixel and the second GEMM sums over regions through its K axis --
    // the same launches as the plain fold, both GEMMs regions_ times as wide.  Otherwise one attention launch per (image, region)
    // and a blend launch (correct, not fast: only levels whose pixels are no multiple of 32, or whose head geometry the fold declines, come here).
    // IMAGE PROMPT (ip_tokens_ > 0): the same two forms with two segments per image, the text keys of kv_all_ and the
    // IPT image tokens of ip_kv_all_ (same column layout: this block's K | V at my_kv), weights (1, s(pixel)): to_out sees
    // attn(q, K_text, V_text) + s attn(q, K_img, V_img).  Only the fold launch differs (two sources of different lengths).
    const int IPT = ip_tokens_;
    const int RG = IPT > 0 ? 2 : regions_, NR = RG > 0 ? RG : 1;
    const int Lkeys = IPT > 0 ? ctx.w : ctx.w / NR; // keys per prompt
    const float* rgw = nullptr;   // this level's weights, fp32 [L][RG]
    if (RG > 0) {
        int lvl = 0;
        while (lvl < 4 && (cfg_.latent_h >> lvl) != x.h) ++lvl;
        if (lvl == 4 || (cfg_.latent_w >> lvl) != x.w) throw Error(INTERNAL_ERROR, "regional prompts: a transformer off the four UNet levels");
        rgw = IPT > 0 ? ip_w_[lvl] : region_w_[lvl];
    }
    const int NK = heads * 80;
    // sdod_xattn_fold_ok is the fold's whole contract, the launch's and the two GEMMs': what it declines takes the forms below
    const bool xfold = xfold_on && fold && sdod_xattn_fold_ok(heads, d, Lkeys, L) != 0;
    // either form leaves its last GEMM to be emitted once its destination is known: t2 = a[rows][K] . w^T + o2b + t1
    struct { f16* a; int K; const f16* w; GemmOpt o; } xo;
    xo.o.bias = o2b; xo.o.residual = t1.p;
    if (xfold) {
        f16 *w1 = nullptr, *w2 = nullptr;
        float *s1 = nullptr, *t1v = nullptr;
        f16* wq = reinterpret_cast<f16*>(params_[q2w].dev);
        const f16* wo = reinterpret_cast<const f16*>(params_[o2w].dev);
        if (mode_ == REAL) {
            SDOD_HIP_CHECK(hipMalloc((void**)&w1, (size_t)B * NR * NK * C * sizeof(f16)));
            SDOD_HIP_CHECK(hipMalloc((void**)&w2, (size_t)B * NR * NK * C * sizeof(f16)));
            SDOD_HIP_CHECK(hipMalloc((void**)&s1, (size_t)B * NR * NK * sizeof(float)));
            SDOD_HIP_CHECK(hipMalloc((void**)&t1v, (size_t)B * NR * NK * sizeof(float)));
            derived_.push_back(w1); derived_.push_back(w2); derived_.push_back(s1); derived_.push_back(t1v);
            const LnVecs qv = ln_fold_vectors(wq, C, C, C, l2w, l2b, nullptr);
            const f16* kvp = kv_all_;
            const int ldkv = kv_total_, koff = my_kv, Lk = Lkeys, hh = heads, dd = d;
            const float scale = 1.0f / sqrtf((float)d);
            to_static_ = true; // (not emit(): its settle() would put a still pending split-K reduce into the static list)
            const f16* ipkv = ip_kv_all_;
            if (IPT > 0)
                sink().push_back(Op{[=](hipStream_t st) {
                    check_rc(sdod_xattn_fold_ip_f16(kvp, ldkv, koff, koff + C, ipkv, ldkv, koff, koff + C, B, Lk, IPT, wq, C, qv.s, qv.t, wo, C, hh, dd, scale,
                                                    w1, s1, t1v, w2, st));
                }, "xattn_fold", 4.0 * B * RG * NK * (double)C * d, 4.0 * B * RG * NK * C * 2,
                   "C" + std::to_string(C) + " d" + std::to_string(d) + " ip" + std::to_string(IPT)});
            else if (RG > 0)
                sink().push_back(Op{[=](hipStream_t st) {
                    check_rc(sdod_xattn_fold_regions_f16(kvp, ldkv, koff, koff + C, B, RG, Lk, wq, C, qv.s, qv.t, wo, C, hh, dd, scale, w1, s1, t1v, w2, st));
                }, "xattn_fold", 4.0 * B * RG * NK * (double)C * d, 4.0 * B * RG * NK * C * 2,
                   "C" + std::to_string(C) + " d" + std::to_string(d) + " regions" + std::to_string(RG)});
            else
            sink().push_back(Op{[=](hipStream_t st) {
                check_rc(sdod_xattn_fold_f16(kvp, ldkv, koff, koff + C, B, Lk, wq, C, qv.s, qv.t, wo, C, hh, dd, scale, w1, s1, t1v, w2, st));
            }, "xattn_fold", 4.0 * B * NK * (double)C * d, 4.0 * B * NK * C * 2, "C" + std::to_string(C) + " d" + std::to_string(d)});
            to_static_ = false;
        }
        const f16* w1p = mode_ == REAL ? w1 : wq; // (placeholders during the sizing pass)
        const f16* w2p = mode_ == REAL ? w2 : wq;
        const int NKR = NR * NK; // (regions: [region][head][80] columns)
        f16* pb = alloc((size_t)rows * NKR);
        { GemmOpt o; o.ln_s_raw = mode_ == REAL ? s1 : reinterpret_cast<const float*>(wq); o.bias_raw = mode_ == REAL ? t1v : reinterpret_cast<const float*>(wq);
          o.w_img_stride = NKR * C; o.vec_img_stride = NKR; o.softmax_cols = 80; o.rows_per_img = L;
          o.region_w = rgw; o.regions = RG;
          linear_raw(t1.p, rows, C, w1p, C, NKR, pb, o); }
        xo.a = pb; xo.K = NKR; xo.w = w2p;
        xo.o.w_img_stride = C * NKR; xo.o.rows_per_img = L;
    } else if (RG > 0) {
        f16* q2 = alloc((size_t)rows * C);
        behind_ln(t1, l2w, l2b, GemmOpt{}, [&](const f16* a, const GemmOpt& og) { linear(a, rows, C, q2w, C, q2, og); });
        // sdod_attention_f16 steps from image to image by Lk * ldk rows; an (image, region) segment does not: batch 1 each
        f16* ar = alloc((size_t)RG * rows * C);
        for (int b = 0; b < B; ++b)
            for (int r = 0; r < RG; ++r) {
                const bool img_seg = IPT > 0 && r == 1; // (image prompt: segment 1 is image b's tokens)
                const f16* kv = img_seg     ? ip_kv_all_ + (size_t)b * IPT * kv_total_ + my_kv
                                : IPT > 0   ? kv_all_ + (size_t)b * Lkeys * kv_total_ + my_kv
                                            : kv_all_ + (size_t)(b * RG + r) * Lkeys * kv_total_ + my_kv;
                attention(q2 + (size_t)b * L * C, kv, kv + C, ar + ((size_t)r * rows + (size_t)b * L) * C, 1, heads, L, img_seg ? IPT : Lkeys, d, C, kv_total_,
                          kv_total_, C, false);
            }
        release(q2);
        { const int rr = rows, LL = L, CC2 = C;
          emit([=](hipStream_t st) { check_rc(sdod_region_blend_f16(ar, (size_t)rr * CC2, rgw, ar, rr, LL, CC2, RG, st)); }, "region_blend", 2.0 * RG * rows * C,
               (double)(RG + 1) * rows * C * 2, "rows" + std::to_string(rows) + " C" + std::to_string(C) + " regions" + std::to_string(RG)); }
        xo.a = ar; xo.K = C; xo.w = W<f16>(o2w);
    } else {
        f16* q2 = alloc((size_t)rows * C);
        behind_ln(t1, l2w, l2b, GemmOpt{}, [&](const f16* a, const GemmOpt& og) { linear(a, rows, C, q2w, C, q2, og); });
        const int Lk = ctx.w;
        const f16* kv = kv_all_ + my_kv;
        f16* a2 = alloc((size_t)rows * C);
        attention(q2, kv, kv + C, a2, B, heads, L, Lk, d, C, kv_total_, kv_total_, C, false);
        release(q2);
        xo.a = a2; xo.K = C; xo.w = W<f16>(o2w);
        xo.o.wq_scale = qscale_of(o2w); xo.o.wq_off = qoff_of(o2w);
    }
    // t2's place.  Composed: [g | t2] rows of 5C -- attn2.to_out writes its C columns (row stride 5C), the GEGLU projection reads
    // them (LayerNorm folded) and writes the first 4C, the composed Linear reads all 5C.  Otherwise a tensor of its own.
    f16* cat = compose ? alloc((size_t)rows * 5 * C) : nullptr;
    const int ld2 = compose ? 5 * C : 0; // (0 = dense)
    Act t2;
    if (compose) { t2.p = cat + 4 * C; t2.n = B; t2.h = 1; t2.w = L; t2.c = C; }
    else t2 = act(B, 1, L, C);
    xo.o.ldr = compose ? C : 0; xo.o.ldo = ld2;
    linear_raw(xo.a, rows, xo.K, xo.w, xo.K, C, t2.p, xo.o);
    release(xo.a); release(t1);
    // ---- 4. GEGLU feed-forward, fused into the ff.net.0.proj epilogue: the [rows][8C] tensor never exists
    f16* gg = compose ? cat : alloc((size_t)rows * 4 * C);
    { GemmOpt o; o.bias = f1b; o.geglu = true; o.lda = ld2; o.ldo = ld2;
      behind_ln(t2, l3w, l3b, o, [&](const f16* a, const GemmOpt& og) { linear(a, rows, C, f1w, 8 * C, gg, og); }); }
    Act out;
    if (compose) {
        float* bc = nullptr;
        if (mode_ == REAL) {
            SDOD_HIP_CHECK(hipMalloc((void**)&bc, (size_t)C * sizeof(float)));
            derived_.push_back(bc);
            f16* wc = reinterpret_cast<f16*>(params_[f2w].dev);
            compose_jobs_.push_back(ComposeJob{wc, wc + 4 * C, 5 * C, C, C, 4 * C, W<float>(f2b), W<float>(pob), bc});
        }
        out = act(x.n, x.h, x.w, C);
        { GemmOpt o; o.bias_raw = mode_ == REAL ? bc : reinterpret_cast<const float*>(params_[f2w].dev); o.residual = x.p;
          linear_raw(cat, rows, 5 * C, W<f16>(f2w), 5 * C, C, out.p, o); }
        release(cat);
    } else {
        Act t3 = act(B, 1, L, C);
        { GemmOpt o; o.bias = f2b; o.residual = t2.p; linear(gg, rows, 4 * C, f2w, C, t3.p, o); }
        release(gg); release(t2);
        out = act(x.n, x.h, x.w, C);
        { GemmOpt o; o.bias = pob; o.residual = x.p; linear(t3.p, rows, C, pow_, C, out.p, o); }
        release(t3);
    }
    return out;
}

// input_blocks.0.0, the 3x3 convolution on the fp32 NCHW latent (build_unet() has checked the sizes)
Act Graph::unet_conv_in(const float* x_in, const float* cond_in) {
    const int B = batch_, H = cfg_.latent_h, Wd = cfg_.latent_w, LC = cfg_.latent_channels, MC = cfg_.model_channels;
    const int CC = cfg_.concat_channels, CI = LC + CC, wr = wrap_;
    const int ciw = P("input_blocks.0.0.weight", {MC, CI, 3, 3}, PK_CONV3_SMALL), cib = P("input_blocks.0.0.bias", {MC}, PK_VEC);
    Act h = act(B, H, Wd, MC);
    const f16* wp = W<f16>(ciw);
    const float* bp = W<float>(cib);
    f16* hp = h.p;
    const std::string shape = "M" + std::to_string(B * H * Wd) + " N" + std::to_string(MC);
    if (CC > 0) {
        // Cin = 9 from two sources (x | cond), K = 81 -> 96 of the 128-wide packed rows, ONE launch (elementwise.hip: CatSrc)
        emit([=](hipStream_t st) { check_rc(sdod_conv_in_cat_f16(x_in, cond_in, wp, bp, hp, B, H, Wd, LC, CC, MC, st)); }, "conv_in_cat",
             2.0 * B * H * Wd * MC * 96, (double)B * H * Wd * (CI * 4 + MC * 2) + MC * 96 * 2, shape + " K96");
    } else if (MC == 320 || MC == 256 || MC == 128 || MC == 64) {
        // ONE launch: im2col rows built in LDS, the whole [MC][64] weight matrix next to them (elementwise.hip: conv_in_kernel)
        emit([=](hipStream_t st) { check_rc(sdod_conv_in_wrap_f16(x_in, wp, bp, hp, B, H, Wd, LC, MC, 1.0f, wr, st)); }, "conv_in",
             2.0 * B * H * Wd * MC * 64, (double)B * H * Wd * (LC * 4 + MC * 2) + MC * 64 * 2, shape + " K64");
    } else {
        // Cin = 4, any width: im2col to K = 64, then the GEMM
        f16* cols = alloc((size_t)B * H * Wd * 64);
        if (wr != 0) { // the wrapped im2col reads NHWC fp16: sdod_latent_im2col_f16 as the two launches it fuses
            Act xl = act(B, H, Wd, LC);
            emit([=](hipStream_t st) { check_rc(sdod_latent_prep_f16(x_in, nullptr, nullptr, xl.p, B, LC, H * Wd, 1.0f, st)); }, "latent_prep", 0,
                 (double)B * H * Wd * LC * 6);
            emit([=](hipStream_t st) { check_rc(sdod_im2col3x3_small_wrap_f16(xl.p, cols, B, H, Wd, LC, 64, wr, st)); }, "im2col_wrap", 0,
                 (double)B * H * Wd * (LC + 64) * 2);
            release(xl);
        } else {
            emit([=](hipStream_t st) { check_rc(sdod_latent_im2col_f16(x_in, cols, B, H, Wd, LC, 64, 1.0f, st)); }, "latent_im2col", 0,
                 (double)B * H * Wd * (LC * 4 + 64 * 2));
        }
        { GemmOpt o; o.bias = cib; linear(cols, B * H * Wd, 64, ciw, MC, h.p, o); }
        release(cols);
    }
    return h;
}

// cross-attention K/V of ALL transformers of the graph: one GEMM on the text context, re-run only when the context changes
void Graph::kv_all_gemm(const f16* ctx_in) {
    if (mode_ == DECLARE || kv_total_ <= 0) return;
    to_static_ = true;
    GemmOpt okv;
    if (quant_mode()) { okv.wq_scale = qscale_of(group_first("attn2_kv_all")); okv.wq_off = qoff_of(group_first("attn2_kv_all")); }
    linear_raw(ctx_in, batch_ * cfg_.context_len, cfg_.context_dim, reinterpret_cast<const f16*>(group_base("attn2_kv_all")), cfg_.context_dim,
               kv_total_, mode_ == REAL ? kv_all_ : const_cast<f16*>(ctx_in) /* placeholder during the sizing pass */, okv);
    to_static_ = false;
}

void Graph::ip_kv_all_gemm(const f16* ip_ctx_in) {
    if (mode_ == DECLARE || kv_total_ <= 0) return;
    to_static_ = true;
    linear_raw(ip_ctx_in, batch_ * ip_tokens_, cfg_.context_dim, reinterpret_cast<const f16*>(group_base("attn2_kv_ip_all")), cfg_.context_dim,
               kv_total_, mode_ == REAL ? ip_kv_all_ : const_cast<f16*>(ip_ctx_in) /* placeholder during the sizing pass */, GemmOpt{});
    to_static_ = false;
}

Act Graph::unet_encoder(Act h, const Act& ctx, const f16* emb_all, int emb_ld, int& emb_off, const f16* const* feat_in, std::vector<Act>* hs,
                        const std::function<void(int, const Act&)>& on_skip) {
    const int MC = cfg_.model_channels, AR = acfg_.adapter_reps;
    int ch = MC, ds = 1, idx = 1, k = 1;
    auto skip = [&](const Act& t) {
        if (hs) hs->push_back(t);
        else on_skip(k, t);
        ++k;
    };
    for (int level = 0; level < 4; ++level) {
        for (int i = 0; i < 2; ++i) {
            const std::string pfx = "input_blocks." + std::to_string(idx++);
            Act r = res_block(pfx + ".0", h, nullptr, kChMult[level] * MC, emb_all, emb_ld, emb_off);
            if (!hs) release_after_consumer(h); // (the block's input: tail or residual of r's, possibly still split-K, out conv)
            ch = kChMult[level] * MC;
            if (ds <= 4) {
                Act t = spatial_transformer(pfx + ".1", r, ctx);
                release(r);
                r = t;
            }
            h = r;
            if (feat_in && i == 1) {
                // ldm input_blocks.2 / .5 / .8 / .11: h = h + features_adapter[level], BEFORE the tensor becomes a skip (TencentARC
                // openaimodel.py).  An ordinary emit: a split-K reduce still pending on h is flushed in front of it.
                f16* hp = h.p;
                const f16* fp = feat_in[level];
                const size_t per = h.numel() / AR;
                emit([=](hipStream_t st) { check_rc(sdod_add_feature_f16(hp, fp, per, AR, st)); }, "add_feature", 0,
                     (double)h.numel() * 4 + (double)per * 2);
            }
            skip(h);
        }
        if (level != 3) {
            const std::string pfx = "input_blocks." + std::to_string(idx++) + ".0.op";
            quant_rows(h.rows() / 4);
            const int w = P(pfx + ".weight", {ch, ch, 3, 3}, PK_CONV3), b = P(pfx + ".bias", {ch}, PK_VEC);
            GemmOpt o; o.bias = b;
            Act d = conv(h, nullptr, w, ch, 3, 2, false, o);
            if (!hs) release(h);
            h = d;
            skip(h);
            ds *= 2;
        }
    }
    // middle (UNet: h is the last skip and stays on the stack until popped)
    Act r1 = res_block("middle_block.0", h, nullptr, ch, emb_all, emb_ld, emb_off);
    if (!hs) release_after_consumer(h);
    Act t = spatial_transformer("middle_block.1", r1, ctx);
    release(r1);
    Act r2 = res_block("middle_block.2", t, nullptr, ch, emb_all, emb_ld, emb_off);
    release_after_consumer(t); // residual of r2's (possibly still split-K) out conv
    return r2;
}

// numel of ControlNet residual k at this graph's batch: the twelve skip tensors in the order the encoder makes them, then the middle
static const int kCtrlDown[13] = {1, 1, 1, 2, 2, 2, 4, 4, 4, 8, 8, 8, 8};
static const int kCtrlMult[13] = {1, 1, 1, 1, 2, 2, 2, 4, 4, 4, 4, 4, 4};
size_t Graph::control_residual_numel(int k) const {
    return (size_t)batch_ * (cfg_.latent_h / kCtrlDown[k]) * (cfg_.latent_w / kCtrlDown[k]) * kCtrlMult[k] * cfg_.model_channels;
}

void Graph::build_unet() {
    const int B = batch_, H = cfg_.latent_h, Wd = cfg_.latent_w, LC = cfg_.latent_channels;
    const int MC = cfg_.model_channels, EC = 4 * MC, cd = cfg_.context_dim, CL = cfg_.context_len;
    const int CC = cfg_.concat_channels, CI = LC + CC; // inpainting checkpoint: the input convolution also reads CC channels of in3
    SDOD_REQUIRE(LC * 9 <= 64, "latent_channels too large for the small-Cin path");
    // three stride-2 levels down and nearest-2x back up must land on the skip tensors' sizes
    SDOD_REQUIRE(H >= 8 && Wd >= 8 && H % 8 == 0 && Wd % 8 == 0, "the UNet needs latent_h and latent_w to be multiples of 8, at least 8");
    SDOD_REQUIRE(CI * 9 <= 96, "latent_channels + concat_channels too large for the small-Cin path (9 Cin <= 96)");
    SDOD_REQUIRE(CC == 0 || CI * 9 > 64, "concat_channels > 0 needs 9 (latent_channels + concat_channels) > 64 (the K = 96 input convolution)");
    SDOD_REQUIRE(CC == 0 || MC == 320 || MC == 256 || MC == 128 || MC == 64,
                 "concat_channels > 0 needs model_channels 64, 128, 256 or 320 (the one-launch input convolution)");

    if (mode_ != DECLARE) { // widths fixed by the DECLARE pass
        int tot = 0;
        for (auto& rb : unet_res_blocks()) tot += rb.second;
        emb_total_ = tot;
    }
    float* x_in = (float*)io_alloc(inputs_, (size_t)B * LC * H * Wd * sizeof(float));
    f16* temb_in = (f16*)io_alloc(inputs_, (size_t)B * std::max(emb_total_, 1) * sizeof(f16));
    f16* ctx_in = (f16*)io_alloc(inputs_, (size_t)B * CL * cd * sizeof(f16));
    const float* cond_in = CC > 0 ? (const float*)io_alloc(inputs_, (size_t)B * CC * H * Wd * sizeof(float)) : nullptr;
    // T2I-Adapter features: one slot per level behind the other inputs, shared by the AR guidance copies of the batch
    const int AR = acfg_.adapter_reps;
    const f16* feat_in[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int l = 0; AR > 0 && l < 4; ++l)
        feat_in[l] = (const f16*)io_alloc(inputs_, (size_t)(B / AR) * (H >> l) * (Wd >> l) * kChMult[l] * MC * sizeof(f16));
    // ControlNet residuals: 13 slots in skip order and their fp32 scales, behind every other input
    const f16* ctrl_in[13] = {};
    const float* ctrl_scale = nullptr;
    if (ccfg_.control_inputs) {
        for (int k = 0; k < 13; ++k) ctrl_in[k] = (const f16*)io_alloc(inputs_, control_residual_numel(k) * sizeof(f16));
        ctrl_scale = (const float*)io_alloc(inputs_, 13 * sizeof(float));
    }
    // regional prompts: the blend weights of the four levels, fp32 [H / ds * W / ds][regions], behind every other
    // input and shared by all images; "region 0 everywhere" until the caller writes them (sdod_region_weights_f32)
    for (int l = 0; l < 4; ++l) region_w_[l] = nullptr;
    if (regions_ > 0) {
        SDOD_REQUIRE(CL == 77 * regions_, "regional prompts: context_len must be 77 * regions");
        SDOD_REQUIRE(AR == 0 && !ccfg_.control_inputs && CC == 0 && wrap_ == 0 && !quant_mode(),
                     "regional prompts exclude adapter inputs, control inputs, concat_channels, wrap and weight_quant");
        for (int l = 0; l < 4; ++l) {
            const size_t n = (size_t)(H >> l) * (Wd >> l) * regions_;
            float* wp = (float*)io_alloc(inputs_, n * sizeof(float));
            if (mode_ == REAL) {
                std::vector<float> init(n, 0.f);
                for (size_t i = 0; i < n; i += regions_) init[i] = 1.f;
                SDOD_HIP_CHECK(hipMemcpy(wp, init.data(), n * sizeof(float), hipMemcpyHostToDevice));
            }
            region_w_[l] = wp;
        }
    }
    // image prompt: the projected image tokens, static like the text context, and the weights of the two segments at
    // the four levels, fp32 [H / ds * W / ds][2], behind every other input; (1, 0) -- no image prompt -- until the caller writes them
    const f16* ip_ctx_in = nullptr;
    for (int l = 0; l < 4; ++l) ip_w_[l] = nullptr;
    if (ip_tokens_ > 0) {
        SDOD_REQUIRE(CL <= 80, "image prompts: context_len must be <= 80");
        SDOD_REQUIRE(AR == 0 && !ccfg_.control_inputs && CC == 0 && wrap_ == 0 && !quant_mode() && regions_ == 0,
                     "image prompts exclude adapter inputs, control inputs, concat_channels, wrap, weight_quant and regions");
        ip_ctx_in = (const f16*)io_alloc(inputs_, (size_t)B * ip_tokens_ * cd * sizeof(f16));
        for (int l = 0; l < 4; ++l) {
            const size_t n = (size_t)(H >> l) * (Wd >> l) * 2;
            float* wp = (float*)io_alloc(inputs_, n * sizeof(float));
            if (mode_ == REAL) {
                std::vector<float> init(n, 0.f);
                for (size_t i = 0; i < n; i += 2) init[i] = 1.f;
                SDOD_HIP_CHECK(hipMemcpy(wp, init.data(), n * sizeof(float), hipMemcpyHostToDevice));
            }
            ip_w_[l] = wp;
        }
    }
    // FreeU: b1, s1, b2, s2 and the version, fp32, behind every other input; the identity until the caller writes them
    const float* freeu_params = nullptr;
    if (freeu_) {
        if (mode_ == REAL) freeu_input_ = (int)inputs_.size();
        float* fp = (float*)io_alloc(inputs_, SDOD_FREEU_PARAMS * sizeof(float));
        if (mode_ == REAL) {
            const float init[SDOD_FREEU_PARAMS] = {1.f, 1.f, 1.f, 1.f, 2.f, 0.f, 0.f, 0.f};
            SDOD_HIP_CHECK(hipMemcpy(fp, init, sizeof(init), hipMemcpyHostToDevice));
        }
        freeu_params = fp;
    }
    f16* e_out = (f16*)io_alloc(outputs_, (size_t)B * H * Wd * LC * sizeof(f16));
    Act ctx;
    ctx.p = ctx_in; ctx.n = B; ctx.h = 1; ctx.w = CL; ctx.c = cd;
    (void)EC;
    // the time conditioning arrives already projected for every ResBlock (TEMB graph): row b, columns [off, off+cout)
    const int emb_ld = emb_total_;
    const f16* emb_all = temb_in;
    int emb_off = 0;
    kv_off_ = 0;
    kv_all_gemm(ctx_in);
    if (ip_tokens_ > 0) ip_kv_all_gemm(ip_ctx_in);

    Act h = unet_conv_in(x_in, cond_in);
    std::vector<Act> hs;
    hs.push_back(h);
    h = unet_encoder(h, ctx, emb_all, emb_ld, emb_off, AR > 0 ? feat_in : nullptr, &hs, nullptr);
    int ch = h.c, ds = 8;
    if (ccfg_.control_inputs) {
        // cldm's ControlledUnetModel: h + control[12] and, where the decoder pops them, hs[k] + control[k].  Every encoder launch has
        // been recorded by now, so the twelve skips take their residual in place, here, in the one launch that also updates h.
        // emit() settles first: a split-K reduce still pending on h (or one that reads a skip tensor as its residual) runs in front
        // of the launch and parked tensors go back to the arena, so nothing reads or writes these tensors behind it but the decoder.
        if (hs.size() != 12) throw Error(INTERNAL_ERROR, "the UNet encoder must leave twelve skip tensors");
        std::vector<sdod_control_seg> segs;
        double by = 0;
        for (int k = 0; k < 13; ++k) {
            const Act& a = k < 12 ? hs[k] : h;
            if (control_residual_numel(k) != a.numel()) throw Error(INTERNAL_ERROR, "control residual shape mismatch");
            segs.push_back(sdod_control_seg{a.p, ctrl_in[k], a.numel()});
            by += (double)a.numel() * 6;
        }
        emit([=](hipStream_t st) { check_rc(sdod_add_control_f16(segs.data(), 13, ctrl_scale, st)); }, "add_control", 0, by);
    }
    int oidx = 0;
    for (int level = 3; level >= 0; --level) {
        for (int i = 0; i < 3; ++i) {
            const std::string pfx = "output_blocks." + std::to_string(oidx++);
            Act skip = hs.back();
            hs.pop_back();
            // FreeU's channel rule on the two tensors about to be concatenated: 4 MC | 4 MC is stage 1, 2 MC | 2 MC stage 2 (the SD
            // shape: output_blocks 0 .. 4 and 7).  The control additions, if any, have run; emit() settles what is pending on h.
            if (freeu_ && h.c == skip.c && (h.c == 4 * MC || h.c == 2 * MC)) freeu_site(h, skip, freeu_params, h.c == 4 * MC ? 1 : 2);
            Act r = res_block(pfx + ".0", h, &skip, kChMult[level] * MC, emb_all, emb_ld, emb_off);
            release(h); release(skip);
            ch = kChMult[level] * MC;
            int sub = 1;
            if (ds <= 4) {
                Act t = spatial_transformer(pfx + "." + std::to_string(sub++), r, ctx);
                release(r);
                r = t;
            }
            if (level != 0 && i == 2) {
                const std::string up = pfx + "." + std::to_string(sub) + ".conv";
                quant_rows(r.rows() * 4);
                const int w = P(up + ".weight", {ch, ch, 3, 3}, PK_CONV3), b = P(up + ".bias", {ch}, PK_VEC);
                GemmOpt o; o.bias = b;
                Act u = conv(r, nullptr, w, ch, 3, 1, true, o);
                release(r);
                r = u;
                ds /= 2;
            }
            h = r;
        }
    }
    const int ow = P("out.0.weight", {ch}, PK_VEC), ob = P("out.0.bias", {ch}, PK_VEC);
    quant_rows(h.rows());
    const int cw = P("out.2.weight", {LC, ch, 3, 3}, PK_CONV3), cb = P("out.2.bias", {LC}, PK_VEC);
    Act g = group_norm(h, nullptr, ow, ob, 1e-5f, true);
    release(h);
    { GemmOpt o; o.bias = cb; o.out = e_out; conv(g, nullptr, cw, LC, 3, 1, false, o); }
    release(g);
    if (mode_ == DECLARE) kv_total_ = kv_off_;
    else if (emb_off != emb_total_ || kv_off_ != kv_total_) throw Error(INTERNAL_ERROR, "UNet conditioning bookkeeping mismatch");
}

// one FreeU site: launch A (skip's low-pass, h's channel means), launch B (h's backbone factor); the means live in the arena between them
void Graph::freeu_site(const Act& h, const Act& skip, const float* params, int stage) {
    if (h.n != skip.n || h.h != skip.h || h.w != skip.w) throw Error(INTERNAL_ERROR, "FreeU site: backbone and skip differ in shape");
    float* means = reinterpret_cast<float*>(alloc((size_t)h.rows() * 2));
    f16* hp = h.p;
    f16* sp = skip.p;
    const int n = h.n, hh = h.h, ww = h.w, c = h.c;
    const std::string shape = "n" + std::to_string(n) + " hw" + std::to_string(hh * ww) + " c" + std::to_string(c) + " stage" + std::to_string(stage);
    const double numel = (double)h.numel();
    emit([=](hipStream_t st) { check_rc(sdod_freeu_f16(hp, sp, n, hh, ww, c, params, stage, means, 1, st)); }, "freeu_filter", 0,
         numel * 6 + (double)h.rows() * 4, shape);
    emit([=](hipStream_t st) { check_rc(sdod_freeu_f16(hp, sp, n, hh, ww, c, params, stage, means, 2, st)); }, "freeu_scale", 0,
         numel * 2 + (double)h.rows() * 4, shape);
    release(means);
}

// (prefix, cout) of every ResBlock in the order build_unet() visits them: the column layout of the TEMB graph's output
std::vector<std::pair<std::string, int>> Graph::unet_res_blocks() const {
    std::vector<std::pair<std::string, int>> v;
    const int MC = cfg_.model_channels;
    int idx = 1;
    for (int level = 0; level < 4; ++level) {
        for (int i = 0; i < 2; ++i) v.emplace_back("input_blocks." + std::to_string(idx++) + ".0", kChMult[level] * MC);
        if (level != 3) ++idx;
    }
    v.emplace_back("middle_block.0", 4 * MC);
    v.emplace_back("middle_block.2", 4 * MC);
    int oidx = 0;
    for (int level = 3; level >= 0; --level)
        for (int i = 0; i < 3; ++i) v.emplace_back("output_blocks." + std::to_string(oidx++) + ".0", kChMult[level] * MC);
    return v;
}

std::vector<std::pair<std::string, int>> Graph::temb_blocks() const {
    auto v = unet_res_blocks();
    if (ccfg_.control_temb || kind_ == SDOD_GRAPH_CONTROLNET) v.resize(10); // a ControlNet has the 8 input and 2 middle ResBlocks only
    return v;
}

// ------------------------------------------------------------------------------------------------ ControlNet
// ldm's cldm.ControlNet for SD 1.x: the UNet's encoder half on weights of its own, the guided hint added behind
// input_blocks.0, and a 1x1 "zero convolution" on each of the twelve skip tensors and on the middle output.  A zero conv writes its
// output slot directly (which sdod_graph_bind_output can point at the UNet's residual input).  No skip stack: a skip tensor goes
// back to the arena once its zero conv and the next block have read it.
void Graph::build_controlnet() {
    const int B = batch_, H = cfg_.latent_h, Wd = cfg_.latent_w, LC = cfg_.latent_channels;
    const int MC = cfg_.model_channels, cd = cfg_.context_dim, CL = cfg_.context_len;
    SDOD_REQUIRE(LC * 9 <= 64, "latent_channels too large for the small-Cin path");
    SDOD_REQUIRE(H >= 8 && Wd >= 8 && H % 8 == 0 && Wd % 8 == 0, "the ControlNet needs latent_h and latent_w to be multiples of 8, at least 8");
    if (mode_ != DECLARE) {
        int tot = 0;
        for (auto& rb : temb_blocks()) tot += rb.second;
        emb_total_ = tot;
    }
    float* x_in = (float*)io_alloc(inputs_, (size_t)B * LC * H * Wd * sizeof(float));
    f16* temb_in = (f16*)io_alloc(inputs_, (size_t)B * std::max(emb_total_, 1) * sizeof(f16));
    f16* ctx_in = (f16*)io_alloc(inputs_, (size_t)B * CL * cd * sizeof(f16));
    const f16* hint_in = (const f16*)io_alloc(inputs_, (size_t)(B / 2) * H * Wd * MC * sizeof(f16));
    f16* outs[13];
    for (int k = 0; k < 13; ++k) outs[k] = (f16*)io_alloc(outputs_, control_residual_numel(k) * sizeof(f16));
    Act ctx;
    ctx.p = ctx_in; ctx.n = B; ctx.h = 1; ctx.w = CL; ctx.c = cd;
    int emb_off = 0;
    kv_off_ = 0;
    kv_all_gemm(ctx_in);

    auto zero_conv = [&](int k, const Act& t) {
        const std::string pfx = k < 12 ? "zero_convs." + std::to_string(k) + ".0" : std::string("middle_block_out.0");
        const int w = P(pfx + ".weight", {t.c, t.c, 1, 1}, PK_CONV1), b = P(pfx + ".bias", {t.c}, PK_VEC);
        if (control_residual_numel(k) != t.numel()) throw Error(INTERNAL_ERROR, "control residual shape mismatch");
        GemmOpt o; o.bias = b;
        linear(t.p, t.rows(), t.c, w, t.c, outs[k], o);
    };
    Act h = unet_conv_in(x_in, nullptr);
    {
        f16* hp = h.p;
        const size_t per = h.numel() / 2;
        emit([=](hipStream_t st) { check_rc(sdod_add_feature_f16(hp, hint_in, per, 2, st)); }, "add_feature", 0, (double)h.numel() * 4 + (double)per * 2);
    }
    zero_conv(0, h);
    h = unet_encoder(h, ctx, temb_in, emb_total_, emb_off, nullptr, nullptr, zero_conv);
    zero_conv(12, h);
    release(h);
    if (mode_ == DECLARE) kv_total_ = kv_off_;
    else if (emb_off != emb_total_ || kv_off_ != kv_total_) throw Error(INTERNAL_ERROR, "ControlNet conditioning bookkeeping mismatch");
}

// cldm's input_hint_block on u / 255: conv 3->16, 16->16, 16->32 /2, 32->32, 32->96 /2, 96->96, 96->256 /2, 256->MC, SiLU behind all but
// the last.  The narrow widths are declared zero-padded (16, 32 -> 64; 96 -> 128) so that every gather GEMM has K % 64 == 0; the
// padded channels stay exactly zero (zero weights, zero bias, SiLU(0) = 0).  The first convolution is the one-launch image input
// convolution in its u / 255 form (its border is zero in the normalised space), SiLU behind it as a launch of its own; the others
// carry SiLU in the GEMM epilogue and the last one writes the output slot.
void Graph::build_control_hint() {
    const int B = batch_, H = cfg_.latent_h, Wd = cfg_.latent_w, MC = cfg_.model_channels;
    SDOD_REQUIRE(H >= 1 && Wd >= 1 && H <= 256 && Wd <= 256, "the hint encoder needs latent_h and latent_w in [1, 256]");
    const int IH = 8 * H, IW = 8 * Wd;
    const uint8_t* img_in = (const uint8_t*)io_alloc(inputs_, (size_t)B * IH * IW * 3);
    f16* out = (f16*)io_alloc(outputs_, (size_t)B * H * Wd * MC * sizeof(f16));
    static const int cpad[8] = {3, 64, 64, 64, 64, 128, 128, 256}; // input width of convolution j as built
    static const int stride[8] = {1, 1, 2, 1, 2, 1, 2, 1};
    const int w0 = P("input_hint_block.0.weight", {cpad[1], 3, 3, 3}, PK_CONV3_SMALL), b0 = P("input_hint_block.0.bias", {cpad[1]}, PK_VEC);
    Act h = act(B, IH, IW, cpad[1]);
    {
        const f16* wp = W<f16>(w0);
        const float* bp = W<float>(b0);
        f16* hp = h.p;
        const size_t cnt = h.numel();
        const int c1 = cpad[1];
        emit([=](hipStream_t st) { check_rc(sdod_image_conv_in_unit_f16(img_in, wp, bp, hp, nullptr, 0, B, IH, IW, c1, st)); }, "image_conv_in_unit",
             2.0 * B * IH * IW * c1 * 64, (double)B * IH * IW * (3 + c1 * 2) + c1 * 64 * 2);
        emit([=](hipStream_t st) { check_rc(sdod_act_f16(hp, hp, cnt, SDOD_ACT_SILU, st)); }, "silu", 0, (double)cnt * 4);
    }
    for (int j = 1; j < 8; ++j) {
        const std::string pfx = "input_hint_block." + std::to_string(2 * j);
        const int cout = j < 7 ? cpad[j + 1] : MC;
        const int w = P(pfx + ".weight", {cout, cpad[j], 3, 3}, PK_CONV3), b = P(pfx + ".bias", {cout}, PK_VEC);
        GemmOpt o; o.bias = b;
        if (j < 7) o.act = SDOD_ACT_SILU;
        else o.out = out;
        Act y = conv(h, nullptr, w, cout, 3, stride[j], false, o);
        release(h);
        h = y;
    }
    if (mode_ != DECLARE) SDOD_REQUIRE(h.h == H && h.w == Wd, "hint size must be 8x the latent size");
}

// ------------------------------------------------------------------------------------------------ temb
void Graph::build_temb() {
    // context.cpp:257-278 (sinusoid -> time MLP), extended by everything else that depends on t only: SiLU and the
    // emb_layers projection of all 22 ResBlocks, as ONE GEMM.  Output row = what the UNet graph consumes as in1.
    const int B = batch_, MC = cfg_.model_channels, EC = 4 * MC;
    const auto blocks = temb_blocks(); // (control_temb: a ControlNet checkpoint's own time_embed and its ten ResBlocks)
    int total = 0;
    for (auto& rb : blocks) total += rb.second;
    float* t_in = (float*)io_alloc(inputs_, (size_t)B * sizeof(float));
    f16* out = (f16*)io_alloc(outputs_, (size_t)B * total * sizeof(f16));
    const int w0 = P("time_embed.0.weight", {EC, MC}, PK_LINEAR), b0 = P("time_embed.0.bias", {EC}, PK_VEC);
    const int w2 = P("time_embed.2.weight", {EC, EC}, PK_LINEAR), b2 = P("time_embed.2.bias", {EC}, PK_VEC);
    for (auto& rb : blocks) {
        P(rb.first + ".emb_layers.1.weight", {rb.second, EC}, PK_LINEAR, "emb_w");
        P(rb.first + ".emb_layers.1.bias", {rb.second}, PK_VEC, "emb_b");
    }
    // a full LCM checkpoint's guidance-scale embedding (sdod_graph_create_lcm): in1 = w, and cond_proj [MC][GD] without a bias, its rows
    // padded to the GEMM's K step where GD is no multiple of it (the padding columns stay zero: allocate_weights clears the arena)
    const int GD = cond_proj_dim_, GK = (GD + 63) / 64 * 64;
    const float* w_in = GD ? (const float*)io_alloc(inputs_, (size_t)B * sizeof(float)) : nullptr;
    const int wc = !GD ? -1 : GK == GD ? P("time_embed.cond_proj.weight", {MC, GD}, PK_LINEAR)
                                       : Pc("time_embed.cond_proj.weight", {MC, GD}, PK_LINEAR, GK, 0, -1);
    f16* feat = alloc((size_t)B * MC);
    f16 *gfeat = nullptr, *tfeat = nullptr; // (held to the end like the other intermediates: the GEMM's residual must outlive its launches)
    emit([=](hipStream_t st) { check_rc(sdod_timestep_features_f16(t_in, feat, B, MC, st)); });
    if (GD) { // feat = timestep_features(t) + guidance_features(w) @ cond_proj^T: the sum rides in the GEMM's residual epilogue
        gfeat = alloc((size_t)B * GK);
        emit([=](hipStream_t st) { sdod::guidance_features_ld(w_in, gfeat, B, GD, GK, st); });
        tfeat = feat;
        feat = alloc((size_t)B * MC);
        { GemmOpt o; o.residual = tfeat; linear(gfeat, B, GK, wc, MC, feat, o); }
    }
    f16* hmid = alloc((size_t)B * EC);
    { GemmOpt o; o.bias = b0; o.act = SDOD_ACT_SILU; linear(feat, B, MC, w0, EC, hmid, o); }
    f16* emb = alloc((size_t)B * EC);
    { GemmOpt o; o.bias = b2; o.act = SDOD_ACT_SILU; linear(hmid, B, EC, w2, EC, emb, o); } // SiLU(time_embed(t)): emb_layers.0
    if (mode_ != DECLARE) {
        GemmOpt o;
        o.bias_raw = reinterpret_cast<const float*>(group_base("emb_b"));
        if (quant_mode()) { o.wq_scale = qscale_of(group_first("emb_w")); o.wq_off = qoff_of(group_first("emb_w")); }
        linear_raw(emb, B, EC, reinterpret_cast<const f16*>(group_base("emb_w")), EC, total, out, o);
    }
    release(feat); release(hmid); release(emb);
    if (GD) { release(gfeat); release(tfeat); }
}

// ------------------------------------------------------------------------------------------------ VAE
Act Graph::vae_res_block(const std::string& pfx, const Act& x, int cout) {
    const int cin = x.c;
    const int n1w = P(pfx + ".norm1.weight", {cin}, PK_VEC), n1b = P(pfx + ".norm1.bias", {cin}, PK_VEC);
    const int c1w = P(pfx + ".conv1.weight", {cout, cin, 3, 3}, PK_CONV3), c1b = P(pfx + ".conv1.bias", {cout}, PK_VEC);
    const int n2w = P(pfx + ".norm2.weight", {cout}, PK_VEC), n2b = P(pfx + ".norm2.bias", {cout}, PK_VEC);
    const int c2w = P(pfx + ".conv2.weight", {cout, cout, 3, 3}, PK_CONV3), c2b = P(pfx + ".conv2.bias", {cout}, PK_VEC);
    int skw = -1, skb = -1;
    if (cin != cout) {
        skw = P(pfx + ".nin_shortcut.weight", {cout, cin, 1, 1}, PK_CONV1);
        skb = P(pfx + ".nin_shortcut.bias", {cout}, PK_VEC);
    }
    Act g1 = group_norm(x, nullptr, n1w, n1b, 1e-6f, true);
    GemmOpt o1; o1.bias = c1b;
    Act h = conv(g1, nullptr, c1w, cout, 3, 1, false, o1);
    release(g1);
    Act g2 = group_norm(h, nullptr, n2w, n2b, 1e-6f, true);
    release(h);
    Act s;
    GemmOpt o2; o2.bias = c2b;
    if (cin != cout) {
        s = act(x.n, x.h, x.w, cout);
        GemmOpt os; os.bias = skb;
        linear(x.p, x.rows(), cin, skw, cout, s.p, os);
        o2.residual = s.p;
    } else {
        o2.residual = x.p;
    }
    Act out = conv(g2, nullptr, c2w, cout, 3, 1, false, o2);
    release(g2);
    if (s.p) release_after_consumer(s);
    return out;
}

Act Graph::vae_attn_block(const std::string& pfx, const Act& x) {
    const int C = x.c, L = x.h * x.w, B = x.n, rows = x.rows();
    const int nw = P(pfx + ".norm.weight", {C}, PK_VEC), nb = P(pfx + ".norm.bias", {C}, PK_VEC);
    const std::string gw = pfx + ".qk_w", gb = pfx + ".qk_b";
    P(pfx + ".q.weight", {C, C, 1, 1}, PK_CONV1, gw);
    P(pfx + ".k.weight", {C, C, 1, 1}, PK_CONV1, gw);
    P(pfx + ".q.bias", {C}, PK_VEC, gb);
    P(pfx + ".k.bias", {C}, PK_VEC, gb);
    const int vw = P(pfx + ".v.weight", {C, C, 1, 1}, PK_CONV1), vb = P(pfx + ".v.bias", {C}, PK_VEC);
    const int pw = P(pfx + ".proj_out.weight", {C, C, 1, 1}, PK_CONV1), pb = P(pfx + ".proj_out.bias", {C}, PK_VEC);
    if (mode_ == DECLARE) return act(x.n, x.h, x.w, C);
    SDOD_REQUIRE(L % 64 == 0 && L <= 16384, "VAE attention needs H*W % 64 == 0 and <= 16384");

    Act g = group_norm(x, nullptr, nw, nb, 1e-6f, false);
    f16* qk = alloc((size_t)rows * 2 * C);
    { GemmOpt o; o.bias_raw = reinterpret_cast<const float*>(group_base(gb));
      linear_raw(g.p, rows, C, reinterpret_cast<const f16*>(group_base(gw)), C, 2 * C, qk, o); }
    f16* att = alloc((size_t)rows * C);
    for (int b = 0; b < B; ++b) {
        const f16* gb_ = g.p + (size_t)b * L * C;
        f16* vt = alloc((size_t)C * L); // V^T [C][L] = Wv . g_b^T + bv   (bias indexed by the output row)
        { GemmOpt o; o.bias = vb; o.bias_on_m = true;
          linear_raw(W<f16>(vw), C, C, gb_, C, L, vt, o); }
        f16* sc = alloc((size_t)L * L);  // scores, softmaxed in place
        { GemmOpt o; o.alpha = 1.0f / sqrtf((float)C); o.lda = 2 * C;
          linear_raw(qk + (size_t)b * L * 2 * C, L, C, qk + (size_t)b * L * 2 * C + C, 2 * C, L, sc, o); }
        emit([=](hipStream_t st) { check_rc(sdod_softmax_rows_f16(sc, sc, L, L, st)); }, "softmax_rows", 0, 2.0 * L * L * 2);
        linear_raw(sc, L, L, vt, L, C, att + (size_t)b * L * C, GemmOpt{});
        release(sc); release(vt);
    }
    release(qk); release(g);
    Act out = act(x.n, x.h, x.w, C);
    { GemmOpt o; o.bias = pb; o.residual = x.p; linear(att, rows, C, pw, C, out.p, o); }
    release(att);
    return out;
}

void Graph::vae_res_step(const std::string& pfx, Act& h, int cout) {
    Act r = vae_res_block(pfx, h, cout);
    release_after_consumer(h); // residual of r's (possibly still split-K) out conv
    h = r;
}

void Graph::vae_mid(const std::string& pfx, Act& h, int ch) {
    vae_res_step(pfx + ".block_1", h, ch);
    { Act r = vae_attn_block(pfx + ".attn_1", h); release(h); h = r; }
    vae_res_step(pfx + ".block_2", h, ch);
}

void Graph::build_vae() {
    const int B = batch_, H = cfg_.latent_h, Wd = cfg_.latent_w, LC = cfg_.latent_channels, VC = cfg_.vae_channels;
    SDOD_REQUIRE(LC * 9 <= 64, "latent_channels too large for the small-Cin path");
    float* z_in = (float*)io_alloc(inputs_, (size_t)B * LC * H * Wd * sizeof(float));
    f16* img_out = (f16*)io_alloc(outputs_, (size_t)B * (8 * H) * (8 * Wd) * 3 * sizeof(f16));

    const int pqw = P("post_quant_conv.weight", {LC, LC, 1, 1}, PK_MAT_F32), pqb = P("post_quant_conv.bias", {LC}, PK_VEC);
    Act zl = act(B, H, Wd, LC);
    {
        const float* wq = W<float>(pqw); const float* bq = W<float>(pqb);
        emit([=](hipStream_t st) { check_rc(sdod_latent_prep_f16(z_in, wq, bq, zl.p, B, LC, H * Wd, 1.0f / 0.18215f, st)); });
    }
    int ch = VC * kChMult[3];
    const int ciw = P("decoder.conv_in.weight", {ch, LC, 3, 3}, PK_CONV3_SMALL), cib = P("decoder.conv_in.bias", {ch}, PK_VEC);
    f16* cols = alloc((size_t)B * H * Wd * 64);
    const int wr = wrap_;
    emit([=](hipStream_t st) { check_rc(sdod_im2col3x3_small_wrap_f16(zl.p, cols, B, H, Wd, LC, 64, wr, st)); });
    Act h = act(B, H, Wd, ch);
    { GemmOpt o; o.bias = cib; linear(cols, B * H * Wd, 64, ciw, ch, h.p, o); }
    release(cols); release(zl);

    vae_mid("decoder.mid", h, ch);
    for (int level = 3; level >= 0; --level) {
        ch = VC * kChMult[level];
        for (int i = 0; i < 3; ++i) vae_res_step("decoder.up." + std::to_string(level) + ".block." + std::to_string(i), h, ch);
        if (level != 0) {
            const std::string up = "decoder.up." + std::to_string(level) + ".upsample.conv";
            const int w = P(up + ".weight", {ch, ch, 3, 3}, PK_CONV3), b = P(up + ".bias", {ch}, PK_VEC);
            GemmOpt o; o.bias = b;
            Act u = conv(h, nullptr, w, ch, 3, 1, true, o);
            release(h);
            h = u;
        }
    }
    const int nw = P("decoder.norm_out.weight", {ch}, PK_VEC), nb = P("decoder.norm_out.bias", {ch}, PK_VEC);
    const int cw = P("decoder.conv_out.weight", {3, ch, 3, 3}, PK_CONV3), cb = P("decoder.conv_out.bias", {3}, PK_VEC);
    Act g = group_norm(h, nullptr, nw, nb, 1e-6f, true);
    release(h);
    { GemmOpt o; o.bias = cb; o.out = img_out; conv(g, nullptr, cw, 3, 3, 1, false, o); }
    release(g);
}

// The encoder half of first_stage_model (ldm Encoder, ch 128, ch_mult (1, 2, 4, 4), 2 ResBlocks per level, double_z) and its
// quant_conv: uint8 image -> moments = quant_conv(encoder(2 u / 255 - 1)), what ldm's img2img encodes the init image with.
//   * conv_in: normalisation, im2col (K = 27 -> 64) and the MFMA product in one launch (sdod_image_conv_in_f16);
//   * Downsample = F.pad(h, (0, 1, 0, 1)) + 3x3 stride-2 conv: the gather GEMM with pad_mode 1 (no padded copy);
//   * quant_conv (1x1, 8 -> 8) composed into conv_out at finalize (sdod_compose_linear_f16: one fp16 rounding of P . W, bias
//     P b + b_q), then one layout change NHWC fp16 -> NCHW fp32 for the moments.
// masked (SDOD_GRAPH_VAE_ENCODER_MASKED): a second input, the inpainting mask, applied by the input convolution in the normalised space
// (sdod_masked_image_conv_in_f16); every other launch and every parameter is the plain encoder's.
void Graph::build_vae_encoder(bool masked) {
    const int B = batch_, H = cfg_.latent_h, Wd = cfg_.latent_w, LC = cfg_.latent_channels, VC = cfg_.vae_channels;
    const int IH = 8 * H, IW = 8 * Wd, ZC = 2 * LC;
    SDOD_REQUIRE(VC == 64 || VC == 128 || VC == 256 || VC == 320, "vae_channels must be 64, 128, 256 or 320 (image input convolution)");
    uint8_t* img_in = (uint8_t*)io_alloc(inputs_, (size_t)B * IH * IW * 3);
    const uint8_t* mask_in = masked ? (const uint8_t*)io_alloc(inputs_, (size_t)B * IH * IW) : nullptr;
    float* mom_out = (float*)io_alloc(outputs_, (size_t)B * ZC * H * Wd * sizeof(float));

    const int ciw = P("encoder.conv_in.weight", {VC, 3, 3, 3}, PK_CONV3_SMALL), cib = P("encoder.conv_in.bias", {VC}, PK_VEC);
    Act h = act(B, IH, IW, VC);
    {
        const f16* wp = W<f16>(ciw);
        const float* bp = W<float>(cib);
        f16* hp = h.p;
        const double fl = 2.0 * B * IH * IW * VC * 64;
        const std::string shape = "M" + std::to_string(B * IH * IW) + " N" + std::to_string(VC) + " K64";
        if (masked)
            emit([=](hipStream_t st) { check_rc(sdod_masked_image_conv_in_f16(img_in, mask_in, wp, bp, hp, B, IH, IW, VC, st)); },
                 "masked_image_conv_in", fl, (double)B * IH * IW * (4 + VC * 2) + VC * 64 * 2, shape);
        else
            emit([=](hipStream_t st) { check_rc(sdod_image_conv_in_f16(img_in, wp, bp, hp, B, IH, IW, VC, st)); }, "image_conv_in", fl,
                 (double)B * IH * IW * (3 + VC * 2) + VC * 64 * 2, shape);
    }
    int ch = VC;
    for (int level = 0; level < 4; ++level) {
        ch = VC * kChMult[level];
        for (int i = 0; i < 2; ++i) vae_res_step("encoder.down." + std::to_string(level) + ".block." + std::to_string(i), h, ch);
        if (level != 3) {
            const std::string dn = "encoder.down." + std::to_string(level) + ".downsample.conv";
            const int w = P(dn + ".weight", {ch, ch, 3, 3}, PK_CONV3), b = P(dn + ".bias", {ch}, PK_VEC);
            GemmOpt o; o.bias = b; o.pad_mode = 1;
            Act d = conv(h, nullptr, w, ch, 3, 2, false, o);
            release(h);
            h = d;
        }
    }
    if (mode_ != DECLARE) SDOD_REQUIRE(h.h == H && h.w == Wd, "image size must be 8x the latent size");
    vae_mid("encoder.mid", h, ch);
    const int nw = P("encoder.norm_out.weight", {ch}, PK_VEC), nb = P("encoder.norm_out.bias", {ch}, PK_VEC);
    // conv_out [ZC][9 ch] and quant_conv [ZC][ZC] share one [ZC][9 ch + ZC] matrix; the first 9 ch columns become quant_conv . conv_out
    const int ld = 9 * ch + ZC;
    const int cw = Pc("encoder.conv_out.weight", {ZC, ch, 3, 3}, PK_CONV3, ld, 0, -1);
    const int cb = P("encoder.conv_out.bias", {ZC}, PK_VEC);
    Pc("quant_conv.weight", {ZC, ZC, 1, 1}, PK_CONV1, ld, 9 * ch, cw);
    const int qb = P("quant_conv.bias", {ZC}, PK_VEC);
    Act g = group_norm(h, nullptr, nw, nb, 1e-6f, true);
    release(h);
    float* bc = nullptr;
    if (mode_ == REAL) {
        SDOD_HIP_CHECK(hipMalloc((void**)&bc, (size_t)ZC * sizeof(float)));
        derived_.push_back(bc);
        f16* wc = reinterpret_cast<f16*>(params_[cw].dev);
        compose_jobs_.push_back(ComposeJob{wc, wc + 9 * ch, ld, ZC, ZC, 9 * ch, W<float>(cb), W<float>(qb), bc});
    }
    GemmOpt o;
    if (mode_ == REAL) o.bias_raw = bc; else o.bias = cb; // (the sizing passes only need a bias of the same shape)
    Act m = conv(g, nullptr, cw, ZC, 3, 1, false, o);
    release(g);
    {
        const f16* mp = m.p;
        emit([=](hipStream_t st) { check_rc(sdod_nhwc_f16_to_nchw_f32(mp, mom_out, B, ZC, H * Wd, st)); }, "nhwc_to_nchw", 0,
             (double)B * ZC * H * Wd * 6);
    }
    release(m);
}

// ------------------------------------------------------------------------------------------------ T2I-Adapter
// TencentARC's "full" adapter, Adapter(channels=[MC, 2 MC, 4 MC, 4 MC], nums_rb, ksize=1, sk=True, use_conv=False), on a uint8 hint:
//   x = conv_in(pixel_unshuffle8(hint / 255));  for stage i, block j (k = i * nums_rb + j):  x = avg_pool2(x) when i > 0 and j == 0,
//   then x = in_conv(x) where the width changes, then x = block2(relu(block1(x))) + x;  x behind a stage's last block is output i.
// block2 (1x1) carries the residual in its epilogue and a stage's last one writes the output slot itself; ReLU is one in-place
// launch (the GEMM epilogue has no such code, see SDOD_ACT_RELU).  The graph runs once per hint, not once per step.
void Graph::build_adapter() {
    const int B = batch_, H = cfg_.latent_h, Wd = cfg_.latent_w, MC = cfg_.model_channels;
    const int HC = acfg_.adapter_hint_channels, NRB = acfg_.adapter_res_blocks > 0 ? acfg_.adapter_res_blocks : 2;
    SDOD_REQUIRE(H >= 8 && Wd >= 8 && H % 8 == 0 && Wd % 8 == 0, "the adapter needs latent_h and latent_w to be multiples of 8, at least 8");
    const int cin = 64 * HC;
    const int ch[4] = {kChMult[0] * MC, kChMult[1] * MC, kChMult[2] * MC, kChMult[3] * MC};
    const uint8_t* hint = (const uint8_t*)io_alloc(inputs_, (size_t)B * (8 * H) * (8 * Wd) * HC);
    f16* outs[4];
    for (int i = 0; i < 4; ++i) outs[i] = (f16*)io_alloc(outputs_, (size_t)B * (H >> i) * (Wd >> i) * ch[i] * sizeof(f16));

    Act u = act(B, H, Wd, cin);
    {
        f16* up = u.p;
        emit([=](hipStream_t st) { check_rc(sdod_pixel_unshuffle_u8_f16(hint, up, B, H, Wd, HC, 8, st)); }, "pixel_unshuffle", 0,
             (double)u.numel() * 3);
    }
    const int ciw = P("conv_in.weight", {MC, cin, 3, 3}, PK_CONV3), cib = P("conv_in.bias", {MC}, PK_VEC);
    Act x;
    { GemmOpt o; o.bias = cib; x = conv(u, nullptr, ciw, MC, 3, 1, false, o); }
    release(u);
    bool x_in_arena = true; // a stage's output lives in its output slot, not in the arena
    auto drop = [&](const Act& a, bool arena) { if (arena) release(a); };
    for (int i = 0; i < 4; ++i) {
        const int c = ch[i];
        for (int j = 0; j < NRB; ++j) {
            const std::string pfx = "body." + std::to_string(i * NRB + j);
            if (i > 0 && j == 0) {
                Act pl = act(B, x.h / 2, x.w / 2, x.c);
                const f16* xp = x.p;
                f16* pp = pl.p;
                const int xh = x.h, xw = x.w, xc = x.c;
                emit([=](hipStream_t st) { check_rc(sdod_avg_pool2_f16(xp, pp, B, xh, xw, xc, st)); }, "avg_pool2", 0, (double)x.numel() * 2.5);
                drop(x, x_in_arena);
                x = pl;
                x_in_arena = true;
                if (ch[i] != ch[i - 1]) {
                    const int w = P(pfx + ".in_conv.weight", {c, ch[i - 1], 1, 1}, PK_CONV1), b = P(pfx + ".in_conv.bias", {c}, PK_VEC);
                    Act y = act(B, x.h, x.w, c);
                    { GemmOpt o; o.bias = b; linear(x.p, x.rows(), x.c, w, c, y.p, o); }
                    release(x);
                    x = y;
                }
            }
            const int w1 = P(pfx + ".block1.weight", {c, c, 3, 3}, PK_CONV3), b1 = P(pfx + ".block1.bias", {c}, PK_VEC);
            const int w2 = P(pfx + ".block2.weight", {c, c, 1, 1}, PK_CONV1), b2 = P(pfx + ".block2.bias", {c}, PK_VEC);
            Act t;
            { GemmOpt o; o.bias = b1; t = conv(x, nullptr, w1, c, 3, 1, false, o); }
            {
                f16* tp = t.p;
                const size_t cnt = t.numel();
                emit([=](hipStream_t st) { check_rc(sdod_act_f16(tp, tp, cnt, SDOD_ACT_RELU, st)); }, "relu", 0, (double)cnt * 4);
            }
            const bool last = j == NRB - 1;
            Act y;
            y.n = x.n; y.h = x.h; y.w = x.w; y.c = c;
            y.p = last ? outs[i] : alloc(y.numel());
            { GemmOpt o; o.bias = b2; o.residual = x.p; linear(t.p, t.rows(), c, w2, c, y.p, o); }
            release(t);
            drop(x, x_in_arena); // (a split-K reduce still pending on this GEMM reads x: release() flushes it first)
            x = y;
            x_in_arena = !last;
        }
    }
}

// ------------------------------------------------------------------------------------------------ ESRGAN upscaler
void Graph::dense_conv(sdod_dense_conv_desc d, int w, int bias) {
    d.w = params_[w].dev;
    d.bias = W<float>(bias);
    if (mode_ == REAL) SDOD_REQUIRE(sdod_dense_conv3x3_ok(&d) == 1, "dense-block convolution refused by its kernel");
    const double px = (double)d.n * (d.h << d.upsample) * (d.w_in << d.upsample);
    const double by = (double)d.n * d.h * d.w_in * d.cin * 2 + 9.0 * d.cin * d.cout * 2 + px * d.cout * 2 * (1 + (d.res1 ? 1 : 0) + (d.res2 ? 1 : 0));
    emit([d](hipStream_t st) { check_rc(sdod_dense_conv3x3_f16(&d, st)); }, d.cout == 32 ? "dense_conv_n32" : "dense_conv_n64",
         2.0 * px * d.cout * 9.0 * d.cin, by,
         std::string("conv3") + (d.upsample ? "u" : "") + " M" + std::to_string((long long)px) + " N" + std::to_string(d.cout) + " K" +
             std::to_string(9 * d.cin));
}

// ESRGAN's RRDBNet (Wang et al. 2018; basicsr's RRDBNet(3, 3, num_feat=64, num_block, num_grow_ch=32, scale=4)) on u / 255:
//   f = conv_first(x);  t = f;  per block: t = RRDB(t);  f = f + conv_body(t);
//   f = lrelu(conv_up1(up2(f)));  f = lrelu(conv_up2(up2(f)));  out = conv_last(lrelu(conv_hr(f)))        (lrelu: slope 0.2)
//   RDB(x): x1..x4 = lrelu(conv_k(x | x1 | ..)), x5 = conv5(x | x1..x4), 0.2 x5 + x;   RRDB(x) = 0.2 RDB3(RDB2(RDB1(x))) + x
// Buffer plan: three [B H W][192] buffers, one per RDB of a block.  A buffer's channels [0, 64) are the RDB's input and convolution k
// writes x_k into channels [64 + 32 (k - 1), 64 + 32 k) of the same buffer, so the concat is the buffer itself; conv5 writes the RDB's
// output (residual in the epilogue) into channels [0, 64) of the next buffer, and the third RDB's conv5 folds the RRDB residual and
// writes the block's output over the block's input in the first buffer (y = 0.04 (acc + b) + 0.2 x3 + x0).  No concat, activation or
// add launch: 15 launches per block.  conv_first keeps a dense copy of its output for conv_body's skip; nearest-2x is folded into
// conv_up1 / conv_up2 (the dense-block kernel with cin = 64); conv_last (64 -> 3) is the gather GEMM.  15 num_blocks + 6 launches.
void Graph::build_upscaler() {
    const int B = batch_, H = ucfg_.in_h, Wd = ucfg_.in_w, NB = ucfg_.num_blocks;
    constexpr int NF = 64, GC = 32, LD = NF + 4 * GC;
    const uint8_t* img_in = (const uint8_t*)io_alloc(inputs_, (size_t)B * H * Wd * 3);
    f16* img_out = (f16*)io_alloc(outputs_, (size_t)B * (4 * H) * (4 * Wd) * 3 * sizeof(f16));
    const size_t rows = (size_t)B * H * Wd;

    const int cfw = P("conv_first.weight", {NF, 3, 3, 3}, PK_CONV3_SMALL), cfb = P("conv_first.bias", {NF}, PK_VEC);
    Act feat = act(B, H, Wd, NF);
    f16* buf[3];
    for (int i = 0; i < 3; ++i) buf[i] = alloc(rows * LD);
    {
        const f16* wp = W<f16>(cfw);
        const float* bp = W<float>(cfb);
        f16 *fp = feat.p, *b0 = buf[0];
        emit([=](hipStream_t st) { check_rc(sdod_image_conv_in_unit_f16(img_in, wp, bp, fp, b0, LD, B, H, Wd, NF, st)); }, "image_conv_in_unit",
             2.0 * rows * NF * 64, (double)rows * (3 + NF * 4) + NF * 64 * 2);
    }
    auto dc = [&](const f16* in, int ld_in, int cin, int w, int b, f16* out, int ld_out, int out_col, int cout, int h, int wd, int ups, float alpha,
                  float slope, const f16* r1, int ld1, float c1, const f16* r2, int ld2) {
        sdod_dense_conv_desc d{};
        d.in = in; d.out = out; d.res1 = r1; d.res2 = r2;
        d.ld_in = ld_in; d.ld_out = ld_out; d.ld_res1 = ld1; d.ld_res2 = ld2;
        d.out_col = out_col; d.cin = cin; d.cout = cout;
        d.n = B; d.h = h; d.w_in = wd; d.upsample = ups;
        d.alpha = alpha; d.slope = slope; d.c1 = c1;
        dense_conv(d, w, b);
    };
    for (int blk = 0; blk < NB; ++blk)
        for (int r = 0; r < 3; ++r) {
            const std::string pfx = "body." + std::to_string(blk) + ".rdb" + std::to_string(r + 1) + ".conv";
            f16* cur = buf[r];
            for (int k = 1; k <= 5; ++k) {
                const int cin = NF + GC * (k - 1), cout = k < 5 ? GC : NF;
                const int w = P(pfx + std::to_string(k) + ".weight", {cout, cin, 3, 3}, PK_CONV3), b = P(pfx + std::to_string(k) + ".bias", {cout}, PK_VEC);
                if (k < 5) dc(cur, LD, cin, w, b, cur, LD, cin, cout, H, Wd, 0, 1.0f, 0.2f, nullptr, 0, 0.f, nullptr, 0);
                else if (r < 2) dc(cur, LD, cin, w, b, buf[r + 1], LD, 0, cout, H, Wd, 0, 0.2f, 0.f, cur, LD, 1.0f, nullptr, 0);
                else dc(cur, LD, cin, w, b, buf[0], LD, 0, cout, H, Wd, 0, 0.04f, 0.f, cur, LD, 0.2f, buf[0], LD);
            }
        }
    const int cbw = P("conv_body.weight", {NF, NF, 3, 3}, PK_CONV3), cbb = P("conv_body.bias", {NF}, PK_VEC);
    const int u1w = P("conv_up1.weight", {NF, NF, 3, 3}, PK_CONV3), u1b = P("conv_up1.bias", {NF}, PK_VEC);
    const int u2w = P("conv_up2.weight", {NF, NF, 3, 3}, PK_CONV3), u2b = P("conv_up2.bias", {NF}, PK_VEC);
    const int hrw = P("conv_hr.weight", {NF, NF, 3, 3}, PK_CONV3), hrb = P("conv_hr.bias", {NF}, PK_VEC);
    const int lw = P("conv_last.weight", {3, NF, 3, 3}, PK_CONV3), lb = P("conv_last.bias", {3}, PK_VEC);
    // f = feat + conv_body(trunk): into buffer 1's first rows, dense (buffers 1 and 2 are free once the trunk is done)
    f16* f0 = buf[1];
    dc(buf[0], LD, NF, cbw, cbb, f0, NF, 0, NF, H, Wd, 0, 1.0f, 0.f, feat.p, NF, 1.0f, nullptr, 0);
    release(feat);
    release(buf[0]);
    release(buf[2]);
    Act f1 = act(B, 2 * H, 2 * Wd, NF);
    dc(f0, NF, NF, u1w, u1b, f1.p, NF, 0, NF, H, Wd, 1, 1.0f, 0.2f, nullptr, 0, 0.f, nullptr, 0);
    release(buf[1]);
    Act f2 = act(B, 4 * H, 4 * Wd, NF);
    dc(f1.p, NF, NF, u2w, u2b, f2.p, NF, 0, NF, 2 * H, 2 * Wd, 1, 1.0f, 0.2f, nullptr, 0, 0.f, nullptr, 0);
    release(f1);
    Act f3 = act(B, 4 * H, 4 * Wd, NF);
    dc(f2.p, NF, NF, hrw, hrb, f3.p, NF, 0, NF, 4 * H, 4 * Wd, 0, 1.0f, 0.2f, nullptr, 0, 0.f, nullptr, 0);
    release(f2);
    { GemmOpt o; o.bias = lb; o.out = img_out; o.split_k = 1; conv(f3, nullptr, lw, 3, 3, 1, false, o); }
    release(f3);
}

// ------------------------------------------------------------------------------------------------ CLIP
Act Graph::clip_block(const std::string& pfx, bool oc, Act x, int heads, int inter, bool causal, int mlp_act) {
    const int B = x.n, L = x.w, D = x.c, rows = B * L;
    const int l1w = P(pfx + (oc ? ".ln_1.weight" : ".layer_norm1.weight"), {D}, PK_VEC), l1b = P(pfx + (oc ? ".ln_1.bias" : ".layer_norm1.bias"), {D}, PK_VEC);
    const std::string gw = pfx + ".qkv_w", gb = pfx + ".qkv_b";
    int qkvw = -1, qkvb = -1;
    if (oc) {
        qkvw = P(pfx + ".attn.in_proj_weight", {3 * D, D}, PK_LINEAR);
        qkvb = P(pfx + ".attn.in_proj_bias", {3 * D}, PK_VEC);
    } else {
        for (const char* n : {"q_proj", "k_proj", "v_proj"}) P(pfx + ".self_attn." + n + ".weight", {D, D}, PK_LINEAR, gw);
        for (const char* n : {"q_proj", "k_proj", "v_proj"}) P(pfx + ".self_attn." + n + ".bias", {D}, PK_VEC, gb);
    }
    const int ow = P(pfx + (oc ? ".attn.out_proj.weight" : ".self_attn.out_proj.weight"), {D, D}, PK_LINEAR);
    const int ob = P(pfx + (oc ? ".attn.out_proj.bias" : ".self_attn.out_proj.bias"), {D}, PK_VEC);
    const int l2w = P(pfx + (oc ? ".ln_2.weight" : ".layer_norm2.weight"), {D}, PK_VEC), l2b = P(pfx + (oc ? ".ln_2.bias" : ".layer_norm2.bias"), {D}, PK_VEC);
    const int f1w = P(pfx + (oc ? ".mlp.c_fc.weight" : ".mlp.fc1.weight"), {inter, D}, PK_LINEAR), f1b = P(pfx + (oc ? ".mlp.c_fc.bias" : ".mlp.fc1.bias"), {inter}, PK_VEC);
    const int f2w = P(pfx + (oc ? ".mlp.c_proj.weight" : ".mlp.fc2.weight"), {D, inter}, PK_LINEAR), f2b = P(pfx + (oc ? ".mlp.c_proj.bias" : ".mlp.fc2.bias"), {D}, PK_VEC);
    if (mode_ == DECLARE) return x;
    // both LayerNorms of a block are folded into the Linear that consumes them (as in the UNet's transformer blocks): no
    // LayerNorm launch, no normalised tensor -- 2 x text_layers launches fewer per prompt
    f16* qkv = alloc((size_t)rows * 3 * D);
    if (oc) {
        GemmOpt o; o.bias = qkvb; o.ln_w = l1w; o.ln_b = l1b;
        linear(x.p, rows, D, qkvw, 3 * D, qkv, o);
    } else {
        GemmOpt o; o.bias_raw = reinterpret_cast<const float*>(group_base(gb)); o.ln_w = l1w; o.ln_b = l1b;
        linear_raw(x.p, rows, D, reinterpret_cast<const f16*>(group_base(gw)), D, 3 * D, qkv, o);
    }
    f16* a = alloc((size_t)rows * D);
    attention(qkv, qkv + D, qkv + 2 * D, a, B, heads, L, L, D / heads, 3 * D, 3 * D, 3 * D, D, causal);
    release(qkv);
    Act x1 = act(B, 1, L, D);
    { GemmOpt o; o.bias = ob; o.residual = x.p; linear(a, rows, D, ow, D, x1.p, o); }
    release(a); release(x);
    f16* f = alloc((size_t)rows * inter);
    { GemmOpt o; o.bias = f1b; o.act = mlp_act; o.ln_w = l2w; o.ln_b = l2b; linear(x1.p, rows, D, f1w, inter, f, o); }
    Act x2 = act(B, 1, L, D);
    { GemmOpt o; o.bias = f2b; o.residual = x1.p; linear(f, rows, inter, f2w, D, x2.p, o); }
    release(f); release(x1);
    return x2;
}

void Graph::build_clip() {
    const int B = batch_, L = cfg_.context_len, D = cfg_.context_dim, heads = cfg_.text_heads, NL = cfg_.text_layers;
    const int rows = B * L, inter = 4 * D;
    SDOD_REQUIRE(heads > 0 && D % heads == 0 && D / heads == 64, "text_heads must be positive and divide context_dim into heads of 64");
    int32_t* ids = (int32_t*)io_alloc(inputs_, (size_t)rows * sizeof(int32_t));
    f16* out = (f16*)io_alloc(outputs_, (size_t)rows * D * sizeof(f16));
    // two checkpoint dialects of the same pre-LN causal transformer (sdod_model_config.text_arch): HF CLIPTextModel names with
    // separate q/k/v projections and quick-GELU (SD1.x), or open_clip names with a fused in_proj and erf GELU (SD2.x)
    const bool oc = cfg_.text_arch == 1;
    const int te = P(oc ? "token_embedding.weight" : "text_model.embeddings.token_embedding.weight", {cfg_.vocab_size, D}, PK_EMBED);
    const int pe = P(oc ? "positional_embedding" : "text_model.embeddings.position_embedding.weight", {L, D}, PK_EMBED);
    Act x = act(B, 1, L, D);
    {
        const f16* tp = W<f16>(te); const f16* pp = W<f16>(pe);
        emit([=](hipStream_t st) { check_rc(sdod_embedding_f16(ids, tp, pp, x.p, rows, L, D, st)); });
    }
    for (int l = 0; l < NL; ++l)
        x = clip_block((oc ? "transformer.resblocks." : "text_model.encoder.layers.") + std::to_string(l), oc, x, heads, inter, true,
                       oc ? SDOD_ACT_GELU : SDOD_ACT_QUICK_GELU);
    const int fw = P(oc ? "ln_final.weight" : "text_model.final_layer_norm.weight", {D}, PK_VEC);
    const int fb = P(oc ? "ln_final.bias" : "text_model.final_layer_norm.bias", {D}, PK_VEC);
    {
        const f16* xp = x.p; const float* wp = W<float>(fw); const float* bp = W<float>(fb);
        emit([=](hipStream_t st) { check_rc(sdod_layer_norm_f16(xp, out, wp, bp, rows, D, 1e-5f, st)); }, "layer_norm", 0, 2.0 * rows * D * 2);
    }
    release(x);
}

// ------------------------------------------------------------------------------------------------ image prompt
// HF CLIPVisionModelWithProjection.  The stride-p patch convolution is a GEMM on rows gathered by sdod_patch_embed_u8_f16 (CLIP's
// normalisation included; K = 3 p^2 zero-padded to a multiple of 64, the weight listed padded); sdod_vit_tokens_f16 puts the class
// token in front, adds the positions and applies pre_layrnorm; the blocks are the text tower's, not causal; post_layernorm is folded
// into visual_projection, which reads the class rows only (row stride (P + 1) W) and writes the output slot.
void Graph::build_image_encoder() {
    static const float kMean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, kStd[3] = {0.26862954f, 0.26130258f, 0.27577711f}; // CLIP's
    const int B = batch_, S = vcfg_.image_size, p = vcfg_.patch, D = vcfg_.width, g = S / p, NP = g * g, L = NP + 1;
    const int KP = (3 * p * p + 63) / 64 * 64, PD = vcfg_.proj_dim;
    const uint8_t* img = (const uint8_t*)io_alloc(inputs_, (size_t)B * S * S * 3);
    f16* out = (f16*)io_alloc(outputs_, (size_t)B * PD * sizeof(f16));
    const std::string em = "vision_model.embeddings.";
    const int pw = P(em + "patch_embedding.weight", {D, KP}, PK_LINEAR);
    const int ce = P(em + "class_embedding", {1, D}, PK_EMBED), pe = P(em + "position_embedding.weight", {L, D}, PK_EMBED);
    const int plw = P("vision_model.pre_layrnorm.weight", {D}, PK_VEC), plb = P("vision_model.pre_layrnorm.bias", {D}, PK_VEC);
    f16* cols = alloc((size_t)B * NP * KP);
    emit([=](hipStream_t st) { check_rc(sdod_patch_embed_u8_f16(img, cols, B, S, p, KP, kMean, kStd, st)); }, "patch_embed", 0,
         (double)B * S * S * 3 + (double)B * NP * KP * 2);
    f16* pt = alloc((size_t)B * NP * D);
    linear(cols, B * NP, KP, pw, D, pt, GemmOpt{});
    release(cols);
    Act x = act(B, 1, L, D);
    {
        const f16* cp = W<f16>(ce); const f16* pp = W<f16>(pe); const float* wp = W<float>(plw); const float* bp = W<float>(plb);
        f16* xp = x.p;
        emit([=](hipStream_t st) { check_rc(sdod_vit_tokens_f16(pt, cp, pp, wp, bp, xp, B, NP, D, 1e-5f, st)); }, "vit_tokens", 0, 4.0 * B * L * D);
    }
    release(pt);
    for (int l = 0; l < vcfg_.layers; ++l)
        x = clip_block("vision_model.encoder.layers." + std::to_string(l), false, x, vcfg_.heads, vcfg_.mlp_dim, false,
                       vcfg_.quick_gelu ? SDOD_ACT_QUICK_GELU : SDOD_ACT_GELU);
    const int fw = P("vision_model.post_layernorm.weight", {D}, PK_VEC), fb = P("vision_model.post_layernorm.bias", {D}, PK_VEC);
    const int vp = P("visual_projection.weight", {PD, D}, PK_LINEAR);
    { GemmOpt o; o.ln_w = fw; o.ln_b = fb; o.lda = L * D; linear(x.p, B, D, vp, PD, out, o); }
    release(x);
}

// IP-Adapter's ImageProjModel: LayerNorm(Linear(image_embeds).reshape(T, ctx_dim)) -- a GEMM and a LayerNorm launch into the output slot
void Graph::build_image_proj() {
    const int B = batch_, PD = vcfg_.proj_dim, T = ip_tokens_, cd = cfg_.context_dim;
    const f16* in = (const f16*)io_alloc(inputs_, (size_t)B * PD * sizeof(f16));
    f16* out = (f16*)io_alloc(outputs_, (size_t)B * T * cd * sizeof(f16));
    const int w = P("proj.weight", {T * cd, PD}, PK_LINEAR), b = P("proj.bias", {T * cd}, PK_VEC);
    const int nw = P("norm.weight", {cd}, PK_VEC), nb = P("norm.bias", {cd}, PK_VEC);
    f16* y = alloc((size_t)B * T * cd);
    { GemmOpt o; o.bias = b; linear(in, B, PD, w, T * cd, y, o); }
    {
        const float* wp = W<float>(nw); const float* bp = W<float>(nb);
        const int rows = B * T;
        emit([=](hipStream_t st) { check_rc(sdod_layer_norm_f16(y, out, wp, bp, rows, cd, 1e-5f, st)); }, "layer_norm", 0, 2.0 * rows * cd * 2);
    }
    release(y);
}

} // namespace sdod
