// lora_host_check.cpp -- stand-alone sanitizer check of the host side of the LoRA entry points (no GPU needed): the argument
// validation of sdod_lora_merge_f16 and of sdod_graph_keep_base / sdod_graph_base_bytes / sdod_graph_set_loras, all of which
// return before any device call.  Built with AddressSanitizer + UndefinedBehaviorSanitizer on the host code by
// `make -C stable-diffusion-on-device_amd lora_host_check`, which also runs it; exit status 0 = every call returned what it should.
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
    alignas(16) static unsigned short w[40 * 72 + 8], up[40 * 128], down[128 * 72];
    expect("null w", sdod_lora_merge_f16(nullptr, 40, 72, 72, up, down, 4, 1.0f, 0, 0, nullptr), kInvalid);
    expect("null up", sdod_lora_merge_f16(w, 40, 72, 72, nullptr, down, 4, 1.0f, 0, 0, nullptr), kInvalid);
    expect("null down", sdod_lora_merge_f16(w, 40, 72, 72, up, nullptr, 4, 1.0f, 0, 0, nullptr), kInvalid);
    expect("rank 0", sdod_lora_merge_f16(w, 40, 72, 72, up, down, 0, 1.0f, 0, 0, nullptr), kInvalid);
    expect("rank 129", sdod_lora_merge_f16(w, 40, 72, 72, up, down, 129, 1.0f, 0, 0, nullptr), kInvalid);
    expect("n 0", sdod_lora_merge_f16(w, 0, 72, 72, up, down, 4, 1.0f, 0, 0, nullptr), kInvalid);
    expect("k 36", sdod_lora_merge_f16(w, 40, 36, 36, up, down, 4, 1.0f, 0, 0, nullptr), kInvalid);
    expect("k 0", sdod_lora_merge_f16(w, 40, 0, 72, up, down, 4, 1.0f, 0, 0, nullptr), kInvalid);
    expect("ld < k", sdod_lora_merge_f16(w, 40, 72, 64, up, down, 4, 1.0f, 0, 0, nullptr), kInvalid);
    expect("ld % 8", sdod_lora_merge_f16(w, 40, 72, 76, up, down, 4, 1.0f, 0, 0, nullptr), kInvalid);
    expect("scale inf", sdod_lora_merge_f16(w, 40, 72, 72, up, down, 4, INFINITY, 0, 0, nullptr), kInvalid);
    expect("scale nan", sdod_lora_merge_f16(w, 40, 72, 72, up, down, 4, NAN, 0, 0, nullptr), kInvalid);
    expect("misaligned w", sdod_lora_merge_f16(w + 1, 40, 72, 72, up, down, 4, 1.0f, 0, 0, nullptr), kInvalid);
    expect("conv_cin mismatch", sdod_lora_merge_f16(w, 40, 72, 72, up, down, 4, 1.0f, 16, 0, nullptr), kInvalid);
    expect("conv_cin negative", sdod_lora_merge_f16(w, 40, 72, 72, up, down, 4, 1.0f, -8, 0, nullptr), kInvalid);
    expect("geglu rows", sdod_lora_merge_f16(w, 40, 72, 72, up, down, 4, 1.0f, 0, 1, nullptr), kInvalid);
    expect("scale 0 launches nothing", sdod_lora_merge_f16(w, 40, 72, 72, up, down, 4, 0.0f, 0, 0, nullptr), 0);

    sdod_model_config cfg;
    sdod_model_config_sd14(&cfg);
    cfg.latent_h = cfg.latent_w = 16;
    cfg.weight_quant = 0;
    void* g = nullptr;
    expect("create", sdod_graph_create(&g, SDOD_GRAPH_UNET, &cfg, 2), 0);
    size_t bytes = 1;
    expect("base_bytes", sdod_graph_base_bytes(g, &bytes), 0);
    if (bytes != 0) { std::printf("FAIL base_bytes of a new graph is %zu\n", bytes); ++failures; }
    expect("base_bytes null", sdod_graph_base_bytes(g, nullptr), kInvalid);
    expect("base_bytes null graph", sdod_graph_base_bytes(nullptr, &bytes), kInvalid);
    expect("keep_base null", sdod_graph_keep_base(nullptr), kInvalid);
    expect("keep_base", sdod_graph_keep_base(g), 0);
    expect("keep_base twice", sdod_graph_keep_base(g), 0);
    expect("base_bytes before finalize", sdod_graph_base_bytes(g, &bytes), 0);
    if (bytes != 0) { std::printf("FAIL base_bytes before finalize is %zu\n", bytes); ++failures; }
    std::vector<float> fu(320 * 4, 0.f), fd(4 * 320, 0.f);
    sdod_lora_entry e[2] = {{"input_blocks.1.1.proj_in.weight", fu.data(), fd.data(), SDOD_F32, 4, 1.0f},
                            {"no.such.weight", fu.data(), fd.data(), SDOD_F32, 4, 1.0f}};
    expect("set_loras null graph", sdod_graph_set_loras(nullptr, e, 1, nullptr), kInvalid);
    expect("set_loras not finalized", sdod_graph_set_loras(g, e, 1, nullptr), kInvalid);
    if (!std::strstr(sdod_hip_last_error(), "not finalized")) { std::printf("FAIL message: %s\n", sdod_hip_last_error()); ++failures; }
    expect("set_loras null entries", sdod_graph_set_loras(g, nullptr, 2, nullptr), kInvalid);
    expect("set_loras negative count", sdod_graph_set_loras(g, e, -1, nullptr), kInvalid);
    expect("set_loras empty, not finalized", sdod_graph_set_loras(g, nullptr, 0, nullptr), kInvalid);
    expect("destroy", sdod_graph_destroy(g), 0);
    std::printf(failures ? "lora_host_check: %d failure(s)\n" : "lora_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
