// lycoris_host_check.cpp -- stand-alone sanitizer check of the host side of the LyCORIS entry points (no GPU needed): the argument
// validation of sdod_loha_merge_f16, sdod_lokr_merge_f16 and sdod_graph_set_networks, all of which return before any device call.
// Built with AddressSanitizer + UndefinedBehaviorSanitizer on the host code by
// `make -C stable-diffusion-on-device_amd lycoris_host_check`, which also runs it; exit status 0 = every call returned what it should.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sdod_engine.h"
#include "sdod_hip.h"

extern "C" const char* sdod_hip_last_error(void);

static int failures = 0;
static void expect(const char* what, int got, int want) {
    if (got != want) {
        std::printf("FAIL %s: status %d, expected %d (%s)\n", what, got, want, sdod_hip_last_error());
        ++failures;
    }
}

int main() {
    constexpr int kInvalid = 2; // LIBSDOD_INVALID_ARGUMENT
    // host buffers stand in for device memory: every call below must be refused before anything reads them
    alignas(16) static unsigned short w[40 * 72 + 8], a1[40 * 128], b1[128 * 72], a2[40 * 128], b2[128 * 72], w1[40 * 72], w2[40 * 72];
    auto loha = [&](void* w_, int n, int k, int ld, const void* p1, const void* p2, const void* p3, const void* p4, int rank, float s, int cin,
                    int geglu) { return sdod_loha_merge_f16(w_, n, k, ld, p1, p2, p3, p4, rank, s, cin, geglu, nullptr); };
    expect("loha null w", loha(nullptr, 40, 72, 72, a1, b1, a2, b2, 4, 1.0f, 0, 0), kInvalid);
    expect("loha null w1a", loha(w, 40, 72, 72, nullptr, b1, a2, b2, 4, 1.0f, 0, 0), kInvalid);
    expect("loha null w1b", loha(w, 40, 72, 72, a1, nullptr, a2, b2, 4, 1.0f, 0, 0), kInvalid);
    expect("loha null w2a", loha(w, 40, 72, 72, a1, b1, nullptr, b2, 4, 1.0f, 0, 0), kInvalid);
    expect("loha null w2b", loha(w, 40, 72, 72, a1, b1, a2, nullptr, 4, 1.0f, 0, 0), kInvalid);
    expect("loha rank 0", loha(w, 40, 72, 72, a1, b1, a2, b2, 0, 1.0f, 0, 0), kInvalid);
    expect("loha rank 129", loha(w, 40, 72, 72, a1, b1, a2, b2, 129, 1.0f, 0, 0), kInvalid);
    expect("loha n 0", loha(w, 0, 72, 72, a1, b1, a2, b2, 4, 1.0f, 0, 0), kInvalid);
    expect("loha k 36", loha(w, 40, 36, 36, a1, b1, a2, b2, 4, 1.0f, 0, 0), kInvalid);
    expect("loha k 0", loha(w, 40, 0, 72, a1, b1, a2, b2, 4, 1.0f, 0, 0), kInvalid);
    expect("loha ld < k", loha(w, 40, 72, 64, a1, b1, a2, b2, 4, 1.0f, 0, 0), kInvalid);
    expect("loha ld % 8", loha(w, 40, 72, 76, a1, b1, a2, b2, 4, 1.0f, 0, 0), kInvalid);
    expect("loha scale inf", loha(w, 40, 72, 72, a1, b1, a2, b2, 4, INFINITY, 0, 0), kInvalid);
    expect("loha scale nan", loha(w, 40, 72, 72, a1, b1, a2, b2, 4, NAN, 0, 0), kInvalid);
    expect("loha misaligned w", loha(w + 1, 40, 72, 72, a1, b1, a2, b2, 4, 1.0f, 0, 0), kInvalid);
    expect("loha misaligned factor", loha(w, 40, 72, 72, a1, b1, reinterpret_cast<char*>(a2) + 1, b2, 4, 1.0f, 0, 0), kInvalid);
    expect("loha conv_cin mismatch", loha(w, 40, 72, 72, a1, b1, a2, b2, 4, 1.0f, 16, 0), kInvalid);
    expect("loha conv_cin negative", loha(w, 40, 72, 72, a1, b1, a2, b2, 4, 1.0f, -8, 0), kInvalid);
    expect("loha geglu rows", loha(w, 40, 72, 72, a1, b1, a2, b2, 4, 1.0f, 0, 1), kInvalid);
    expect("loha scale 0 launches nothing", loha(w, 40, 72, 72, a1, b1, a2, b2, 4, 0.0f, 0, 0), 0);

    auto lokr = [&](void* w_, int n, int k, int ld, const void* p1, int a, int b, const void* p2, float s, int cin, int geglu) {
        return sdod_lokr_merge_f16(w_, n, k, ld, p1, a, b, p2, s, cin, geglu, nullptr);
    };
    expect("lokr null w", lokr(nullptr, 40, 72, 72, w1, 8, 8, w2, 1.0f, 0, 0), kInvalid);
    expect("lokr null w1", lokr(w, 40, 72, 72, nullptr, 8, 8, w2, 1.0f, 0, 0), kInvalid);
    expect("lokr null w2", lokr(w, 40, 72, 72, w1, 8, 8, nullptr, 1.0f, 0, 0), kInvalid);
    expect("lokr a 0", lokr(w, 40, 72, 72, w1, 0, 8, w2, 1.0f, 0, 0), kInvalid);
    expect("lokr b 0", lokr(w, 40, 72, 72, w1, 8, 0, w2, 1.0f, 0, 0), kInvalid);
    expect("lokr a negative", lokr(w, 40, 72, 72, w1, -8, 8, w2, 1.0f, 0, 0), kInvalid);
    expect("lokr a does not divide n", lokr(w, 40, 72, 72, w1, 3, 8, w2, 1.0f, 0, 0), kInvalid);
    expect("lokr b does not divide k", lokr(w, 40, 72, 72, w1, 8, 7, w2, 1.0f, 0, 0), kInvalid);
    expect("lokr b divides k but not cin", lokr(w, 40, 72, 72, w1, 8, 9, w2, 1.0f, 8, 0), kInvalid);
    expect("lokr n 0", lokr(w, 0, 72, 72, w1, 1, 8, w2, 1.0f, 0, 0), kInvalid);
    expect("lokr k 36", lokr(w, 40, 36, 36, w1, 8, 4, w2, 1.0f, 0, 0), kInvalid);
    expect("lokr ld < k", lokr(w, 40, 72, 64, w1, 8, 8, w2, 1.0f, 0, 0), kInvalid);
    expect("lokr ld % 8", lokr(w, 40, 72, 76, w1, 8, 8, w2, 1.0f, 0, 0), kInvalid);
    expect("lokr scale inf", lokr(w, 40, 72, 72, w1, 8, 8, w2, INFINITY, 0, 0), kInvalid);
    expect("lokr scale nan", lokr(w, 40, 72, 72, w1, 8, 8, w2, NAN, 0, 0), kInvalid);
    expect("lokr misaligned w", lokr(w + 1, 40, 72, 72, w1, 8, 8, w2, 1.0f, 0, 0), kInvalid);
    expect("lokr conv_cin mismatch", lokr(w, 40, 72, 72, w1, 8, 8, w2, 1.0f, 16, 0), kInvalid);
    expect("lokr geglu rows", lokr(w, 40, 72, 72, w1, 8, 8, w2, 1.0f, 0, 1), kInvalid);
    expect("lokr scale 0 launches nothing", lokr(w, 40, 72, 72, w1, 8, 8, w2, 0.0f, 0, 0), 0);

    sdod_model_config cfg;
    sdod_model_config_sd14(&cfg);
    cfg.latent_h = cfg.latent_w = 16;
    cfg.weight_quant = 0;
    void* g = nullptr;
    expect("create", sdod_graph_create(&g, SDOD_GRAPH_UNET, &cfg, 2), 0);
    expect("keep_base", sdod_graph_keep_base(g), 0);
    std::vector<float> fa(320 * 4, 0.f), fb(4 * 320, 0.f);
    sdod_network_entry e[3] = {
        {"input_blocks.1.1.proj_in.weight", SDOD_NET_LOHA, SDOD_F32, {fa.data(), fb.data(), fa.data(), fb.data()}, 4, 0, 0, 1.0f},
        {"input_blocks.1.1.proj_in.weight", SDOD_NET_LOKR, SDOD_F32, {fa.data(), fb.data(), nullptr, nullptr}, 0, 4, 4, 1.0f},
        {"no.such.weight", SDOD_NET_LORA, SDOD_F32, {fa.data(), fb.data(), nullptr, nullptr}, 4, 0, 0, 1.0f}};
    expect("set_networks null graph", sdod_graph_set_networks(nullptr, e, 1, nullptr), kInvalid);
    expect("set_networks not finalized", sdod_graph_set_networks(g, e, 3, nullptr), kInvalid);
    if (!std::strstr(sdod_hip_last_error(), "not finalized")) { std::printf("FAIL message: %s\n", sdod_hip_last_error()); ++failures; }
    expect("set_networks null entries", sdod_graph_set_networks(g, nullptr, 2, nullptr), kInvalid);
    expect("set_networks negative count", sdod_graph_set_networks(g, e, -1, nullptr), kInvalid);
    expect("set_networks empty, not finalized", sdod_graph_set_networks(g, nullptr, 0, nullptr), kInvalid);
    expect("destroy", sdod_graph_destroy(g), 0);
    std::printf(failures ? "lycoris_host_check: %d failure(s)\n" : "lycoris_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
