// resize_host_check.cpp -- stand-alone sanitizer check of the host side of the latent resize (no GPU needed): the tap table of
// sdod_latent_resize_taps at the edge sizes, and the argument checks of sdod_latent_resize_f32, all of which return before any device
// call.  Built with AddressSanitizer + UndefinedBehaviorSanitizer on the host code by
// `make -C stable-diffusion-on-device_amd resize_host_check`, which also runs it; exit status 0 = every call returned what it should.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sdod_hip.h"

extern "C" const char* sdod_hip_last_error(void);

static int failures = 0;
static void expect(const char* what, int got, int want) {
    if (got != want) {
        std::printf("FAIL %s: status %d, expected %d (%s)\n", what, got, want, sdod_hip_last_error());
        ++failures;
    }
}

// every row of the table: indices inside [0, n_in), finite weights that sum to 1; n -> n: exactly one slot holds index d
// with weight 1, every other slot weight 0.  The vectors are
// sized exactly, so a write past [n_out][4] is the sanitizer's to report.
static void table(int mode, int n_in, int n_out) {
    std::vector<int32_t> idx((size_t)n_out * 4, -1);
    std::vector<float> w((size_t)n_out * 4, NAN);
    char what[64];
    std::snprintf(what, sizeof what, "taps mode %d %d -> %d", mode, n_in, n_out);
    expect(what, sdod_latent_resize_taps(mode, n_in, n_out, idx.data(), w.data()), 0);
    for (int d = 0; d < n_out; ++d) {
        double sum = 0.0;
        int ones = 0;
        for (int k = 0; k < 4; ++k) {
            const int32_t i = idx[(size_t)d * 4 + k];
            const float v = w[(size_t)d * 4 + k];
            if (i < 0 || i >= n_in || !std::isfinite(v)) { std::printf("FAIL %s: row %d slot %d = (%d, %g)\n", what, d, k, i, v); ++failures; }
            if (n_in == n_out && v != 0.0f && (v != 1.0f || i != d)) { std::printf("FAIL %s: row %d is not the identity\n", what, d); ++failures; }
            if (v == 1.0f && i == d) ++ones;
            sum += v;
        }
        if (n_in == n_out && ones != 1) { std::printf("FAIL %s: row %d holds %d taps of weight 1 on index %d\n", what, d, ones, d); ++failures; }
        if (std::fabs(sum - 1.0) > 1e-6) { std::printf("FAIL %s: row %d sums to %.9g\n", what, d, sum); ++failures; }
    }
}

int main() {
    constexpr int kInvalid = 2; // LIBSDOD_INVALID_ARGUMENT
    const int pairs[][2] = {{1, 1}, {1, 2}, {2, 1}, {1, 97}, {97, 1}, {2, 3}, {3, 2}, {5, 13}, {7, 9}, {8, 16}, {16, 24}, {24, 16},
                            {64, 96}, {16, 16}, {4096, 4097}, {46341, 46340}, {1 << 20, 3}, {3, 1 << 16}};
    for (int mode = 0; mode < 3; ++mode)
        for (const auto& p : pairs) table(mode, p[0], p[1]);
    table(2, 2147483647, 5); // (2 d + 1) n_in leaves 32 bits
    table(1, 5, 1 << 22);

    int32_t idx[4];
    float w[4];
    expect("taps null idx", sdod_latent_resize_taps(1, 4, 1, nullptr, w), kInvalid);
    expect("taps null w", sdod_latent_resize_taps(1, 4, 1, idx, nullptr), kInvalid);
    expect("taps mode 3", sdod_latent_resize_taps(3, 4, 1, idx, w), kInvalid);
    expect("taps mode -1", sdod_latent_resize_taps(-1, 4, 1, idx, w), kInvalid);
    expect("taps n_in 0", sdod_latent_resize_taps(1, 0, 1, idx, w), kInvalid);
    expect("taps n_out 0", sdod_latent_resize_taps(1, 4, 0, idx, w), kInvalid);
    expect("taps n_out negative", sdod_latent_resize_taps(1, 4, -3, idx, w), kInvalid);

    // host buffers stand in for device memory: every call below must be refused before anything reads or writes them
    static float src[2 * 4 * 5 * 7], dst[2 * 4 * 13 * 9], both[2 * 4 * 13 * 9 + 2 * 4 * 5 * 7];
    expect("null src", sdod_latent_resize_f32(nullptr, dst, 2, 4, 5, 7, 13, 9, 1, 1.f, 0.f, nullptr, 0, 0, nullptr), kInvalid);
    expect("null dst", sdod_latent_resize_f32(src, nullptr, 2, 4, 5, 7, 13, 9, 1, 1.f, 0.f, nullptr, 0, 0, nullptr), kInvalid);
    expect("n 0", sdod_latent_resize_f32(src, dst, 0, 4, 5, 7, 13, 9, 1, 1.f, 0.f, nullptr, 0, 0, nullptr), kInvalid);
    expect("c 0", sdod_latent_resize_f32(src, dst, 2, 0, 5, 7, 13, 9, 1, 1.f, 0.f, nullptr, 0, 0, nullptr), kInvalid);
    expect("h_in 0", sdod_latent_resize_f32(src, dst, 2, 4, 0, 7, 13, 9, 1, 1.f, 0.f, nullptr, 0, 0, nullptr), kInvalid);
    expect("w_in negative", sdod_latent_resize_f32(src, dst, 2, 4, 5, -7, 13, 9, 1, 1.f, 0.f, nullptr, 0, 0, nullptr), kInvalid);
    expect("h_out 0", sdod_latent_resize_f32(src, dst, 2, 4, 5, 7, 0, 9, 1, 1.f, 0.f, nullptr, 0, 0, nullptr), kInvalid);
    expect("w_out 0", sdod_latent_resize_f32(src, dst, 2, 4, 5, 7, 13, 0, 1, 1.f, 0.f, nullptr, 0, 0, nullptr), kInvalid);
    expect("mode 3", sdod_latent_resize_f32(src, dst, 2, 4, 5, 7, 13, 9, 3, 1.f, 0.f, nullptr, 0, 0, nullptr), kInvalid);
    expect("mode -1", sdod_latent_resize_f32(src, dst, 2, 4, 5, 7, 13, 9, -1, 1.f, 0.f, nullptr, 0, 0, nullptr), kInvalid);
    expect("a nan", sdod_latent_resize_f32(src, dst, 2, 4, 5, 7, 13, 9, 1, NAN, 0.f, nullptr, 0, 0, nullptr), kInvalid);
    expect("b inf", sdod_latent_resize_f32(src, dst, 2, 4, 5, 7, 13, 9, 1, 1.f, INFINITY, nullptr, 0, 0, nullptr), kInvalid);
    expect("dst == src", sdod_latent_resize_f32(both, both, 2, 4, 5, 7, 13, 9, 1, 1.f, 0.f, nullptr, 0, 0, nullptr), kInvalid);
    expect("dst inside src", sdod_latent_resize_f32(both, both + 2 * 4 * 5 * 7 - 1, 2, 4, 5, 7, 13, 9, 1, 1.f, 0.f, nullptr, 0, 0, nullptr), kInvalid);
    expect("src inside dst", sdod_latent_resize_f32(both + 2 * 4 * 13 * 9 - 1, both, 2, 4, 5, 7, 13, 9, 1, 1.f, 0.f, nullptr, 0, 0, nullptr), kInvalid);
    std::printf(failures ? "resize_host_check: %d failure(s)\n" : "resize_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
