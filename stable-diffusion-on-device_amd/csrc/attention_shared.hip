// attention_shared.hip -- shared-key self-attention: every main sequence of a batch attends to its own keys and values
// plus those of an anchor sequence that rides in the same batch.
//
// This is the attention of "reference-only" control (the reference_only preprocessor of A1111's ControlNet extension, diffusers'
// StableDiffusionReferencePipeline with reference_attn, ComfyUI's ReferenceOnly node): a reference picture, noised to the current
// step, goes through the same UNet, and every attn1 of the generated rows sees [K_own ; K_ref], [V_own ; V_ref]; style_fidelity
// mixes the self-only result back in on the uncond rows.  With the reference rows in the UNet batch their K and V already lie in the
// packed qkv buffer the block's GEMM wrote, one batch entry away, so nothing is banked or concatenated: the fused kernel
// (attention_kernel.h) is instantiated a third time with its SHARED parameter and walks a second key segment from another batch entry.
//   * Segments.  The tile loop runs NTG rounds over the own keys and NTG rounds over the anchor's.  A tile is (segment row offset, tile
//     inside the segment): the unpredicated load, the zero fill and the key mask all test the tile against the SEGMENT's length, so a
//     ragged tile in the middle of the walk is masked like a ragged last one.  The deferred shift's "first tile" flag follows the
//     wave group, not the segment: it clears once the group has run a tile.
//   * Blend.  out = w * softmax(q K_own^T) V_own + (1 - w) * softmax(q [K_own ; K_anc]^T) [V_own ; V_anc].  The online softmax's state
//     at the segment boundary IS the first term, so it costs no score work.  For 0 < w < 1 the workgroup writes w * O / l, rounded to
//     fp16, into its own output rows at the boundary and every lane adds its pieces back in the epilogue: no LDS, no register held
//     across the anchor segment, one extra fp16 rounding of the first term (|error| <= 2^-11 w |O_own|).  The alternatives: O in
//     registers is QT * NDT * 4 = 24 more VGPRs at d = 40 and ends three workgroups per CU for EVERY workgroup of the launch; an fp32
//     LDS snapshot is 24 KB beside 30 KB of stages at d = 40 and ends it the same way, again for all of them, since the LDS of a launch
//     is one size; a second instantiation for blending workgroups cannot be chosen per workgroup from a launch argument, and w is
//     deliberately not one.  w == 0, w == 1 and the anchor sequences take none of these paths: the branches are workgroup-uniform.
//   * w == 1 and the anchor sequences walk one segment: the plain kernel's loop, bit for bit what sdod_attention_f16 returns.
//   * Key/value split (d = 80, l >= 256: two groups of four waves).  Each segment is dealt to the groups from its own tile 0, so both
//     groups reach the boundary in the same round; there group 1 parks its (m, l, O) in the stage it has just finished reading, group 0
//     merges on the fly for the snapshot only, and two barriers fence the stage.  With an odd tile count a group idles one round per
//     segment and stages its next tile in that round itself.  w == 0 pays nothing for this.
// self_w lives in device memory and is read by the kernel, so a captured launch follows a new value without a recapture.
//
// Compiled with attention.hip's flags (Makefile), as attention_tiled.hip is and for the same reason.
#include "attention_kernel.h"

extern "C" int sdod_attention_shared_f16(const void* q, const void* k, const void* v, void* out, int batch, int heads, int l, int d,
                                         int ldq, int ldk, int ldv, int ldo, float scale, int anchors, const float* self_w, void* stream) {
    SDOD_TRY
    SDOD_REQUIRE(q && k && v && out && self_w, "null pointer");
    SDOD_REQUIRE(batch > 0 && heads > 0 && l > 0, "bad shape");
    SDOD_REQUIRE(anchors == 1 || anchors == 2, "anchors must be 1 or 2");
    SDOD_REQUIRE(batch > anchors && (batch - anchors) % anchors == 0, "batch - anchors must be a positive multiple of anchors");
    SDOD_ATTN_REQUIRE_OPERANDS(q, k, v, out, heads, d, ldq, ldk, ldv, ldo, scale);
    SDOD_REQUIRE(((uintptr_t)self_w & 3) == 0, "misaligned pointer");
    SDOD_REQUIRE((long long)batch * l <= INT_MAX && (long long)batch * heads * ((l + 63) / 64) <= INT_MAX, "bad shape (too many rows or workgroups)");
    // 0 < w < 1 parks an intermediate in out while other workgroups still read k and v: the address ranges must be apart (w is device
    // memory, so this holds for every w; a w outside [0, 1] or a NaN is not looked at: the formula applies as it stands)
    {
        const size_t rows = (size_t)batch * l - 1, cols = (size_t)heads * d;
        const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (rows * ldo + cols) * sizeof(f16);
        const uintptr_t k0 = (uintptr_t)k, k1 = k0 + (rows * ldk + cols) * sizeof(f16);
        const uintptr_t v0 = (uintptr_t)v, v1 = v0 + (rows * ldv + cols) * sizeof(f16);
        SDOD_REQUIRE((o1 <= k0 || k1 <= o0) && (o1 <= v0 || v1 <= o0), "out must not overlap k or v");
    }
    AttnSP p{};
    p.q = (const f16*)q; p.k = (const f16*)k; p.v = (const f16*)v; p.out = (f16*)out;
    p.B = batch; p.H = heads; p.Lq = p.Lk = l;
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
    p.scale_log2 = scale * 1.4426950408889634f;
    p.causal = 0;
    p.anchors = anchors; p.per = (batch - anchors) / anchors;
    p.self_w = self_w;
    // the form sdod_attention_f16 chooses for `batch` sequences of lq = lk = l: the segments are the same length
    SDOD_HIP_CHECK(attn_run(p, d, (hipStream_t)stream));
    return 0;
    SDOD_CATCH
}
