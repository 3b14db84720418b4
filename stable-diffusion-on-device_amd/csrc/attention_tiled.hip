// attention_tiled.hip -- HyperTile: self-attention inside the th x tw tiles of an h x w token map, in place.
//
// The method (tfernd/HyperTile; "Hypertile" in A1111, the HyperTile node in ComfyUI) rearranges b (nh h nw w) c -> (b nh nw) (h w) c
// around a UNet's attn1, so that every tile is a softmax domain of its own and the score work falls by nh * nw.  The rows of a tile
// lie in runs of tw pixels one map row apart, which no stride of sdod_attention_f16 expresses, and a gather / scatter pair would
// cost two launches and two activation round trips per attention.  So the fused kernel (attention_kernel.h) is instantiated a
// second time with its TILED parameter: same tile loop, same online softmax, same LDS and register layout -- only the three places
// that turn a row index into an address change:
//   * a workgroup owns 64 * QT query rows of one (image, tile, head); its Q fragments and its output rows go through the row map
//     j -> (j / tw) * w + j % tw once;
//   * the staging threads keep, per 16-byte piece, a 32-bit byte offset into K and into V and the key's column x inside the tile,
//     and move them from one 64-key tile to the next by a wave-uniform step and one carry -- no division in the loop, and three
//     registers per piece where the untiled kernel holds two 64-bit pointers;
//   * keys past th * tw are masked by the predicates the kernel already has for ragged sequences.
// The kernel form is chosen by the same function as sdod_attention_f16's (attn_run) for batch = B * nh * nw, lq = lk = th * tw.
//
// This file is compiled with attention.hip's flags (Makefile), and has to be: which of the final fp32 -> fp16 conversions the compiler
// fuses with the normalising multiply (one rounding instead of two) follows the flags, and a tile must equal sdod_attention_f16 on
// its gathered rows bit for bit.
#include "attention_kernel.h"

#include <algorithm>

namespace {
// smallest divisor of n that is >= min(t, n)
int divisor_at_least(int n, int t) {
    int d = std::min(t, n);
    while (n % d != 0) ++d;
    return d;
}
} // namespace

// the tile rule (include/sdod_hip.h): the ONE statement of it.  Host-only.
extern "C" int sdod_hypertile_grid(int h, int w, int tile, int level, int max_depth, int* th, int* tw) {
    SDOD_TRY
    SDOD_REQUIRE(th && tw, "null pointer");
    SDOD_REQUIRE(h > 0 && w > 0, "bad shape");
    SDOD_REQUIRE(tile >= 8, "tile must be >= 8 latent pixels");
    SDOD_REQUIRE(level >= 0 && level <= 30 && max_depth >= 0 && max_depth <= 3, "level must be in [0, 30] and max_depth in [0, 3]");
    *th = *tw = 0; // (an untiled level)
    // the tile COUNT per axis is fixed at level 0 and kept at every level
    const int nh = h / divisor_at_least(h, tile), nw = w / divisor_at_least(w, tile);
    const int hl = h >> level, wl = w >> level;
    if (level > max_depth || nh * nw == 1 || hl == 0 || wl == 0 || hl % nh != 0 || wl % nw != 0) return 0;
    *th = hl / nh;
    *tw = wl / nw;
    return 0;
    SDOD_CATCH
}

extern "C" int sdod_attention_tiled_f16(const void* q, const void* k, const void* v, void* out, int batch, int heads, int h, int w,
                                        int th, int tw, int d, int ldq, int ldk, int ldv, int ldo, float scale, void* stream) {
    SDOD_TRY
    SDOD_REQUIRE(q && k && v && out, "null pointer");
    SDOD_REQUIRE(batch > 0 && heads > 0 && h > 0 && w > 0 && th > 0 && tw > 0, "bad shape");
    SDOD_REQUIRE(h % th == 0 && w % tw == 0, "th must divide h and tw must divide w");
    SDOD_ATTN_REQUIRE_OPERANDS(q, k, v, out, heads, d, ldq, ldk, ldv, ldo, scale);
    // every count the kernel holds in an int, and the 32-bit byte offsets of the staging threads: a piece's offset runs at most one
    // step (128 keys: up to 129 map rows) past a ragged last tile's 63 surplus keys (up to 64 more), all inside 260 map rows
    const long long hw = (long long)h * w, tiles = (long long)(h / th) * (w / tw), L = (long long)th * tw;
    const long long ld_kv = std::max(ldk, ldv);
    SDOD_REQUIRE(hw <= INT_MAX && (long long)batch * hw <= INT_MAX, "bad shape (batch * h * w must fit an int)");
    SDOD_REQUIRE((hw + 260LL * w) * ld_kv < (1LL << 30), "bad shape ((h * w + 260 w) * max(ldk, ldv) must stay below 2^30)");
    SDOD_REQUIRE((long long)batch * tiles * heads * ((L + 63) / 64) <= INT_MAX, "bad shape (too many workgroups)");
    AttnTP p{};
    p.q = (const f16*)q; p.k = (const f16*)k; p.v = (const f16*)v; p.out = (f16*)out;
    p.B = (int)(batch * tiles); p.H = heads; p.Lq = p.Lk = (int)L;
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
    p.scale_log2 = scale * 1.4426950408889634f;
    p.causal = 0;
    p.w = w; p.hw = (int)hw; p.th = th; p.tw = tw;
    p.ntx = w / tw; p.ntiles = (int)tiles;
    for (int kvs = 1; kvs <= 2; ++kvs) {
        p.step_y[kvs - 1] = 64 * kvs / tw;
        p.step_x[kvs - 1] = 64 * kvs % tw;
    }
    SDOD_HIP_CHECK(attn_run(p, d, (hipStream_t)stream));
    return 0;
    SDOD_CATCH
}
