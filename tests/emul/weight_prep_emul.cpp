// CPU check of the host arithmetic of weight upload, the very headers the library compiles:
//   ace_amd/csrc/weight_prep.h  pow2_scale (the power-of-two scale of every static f16x3 operand) and weight_norms (max |w| and the
//                               rounded-up max row sum that bounds a convolution's output)
//   ace_amd/csrc/conv_roles.h   which 1x1-convolution roles conv_ws.hip / conv_wl.hip serve, and on which grid each block asks
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../ace_amd/csrc/conv_roles.h"
#include "../../ace_amd/csrc/weight_prep.h"

using namespace ace;

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++bad; std::printf("FAIL %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

static void check_pow2_scale() {
    std::vector<float> in = {0.f, std::numeric_limits<float>::denorm_min(), FLT_MIN, FLT_MAX, INFINITY, NAN};
    for (int k : {-20, 0, 9, 10, 30}) {
        const float p = std::ldexp(1.0f, k);
        in.push_back(std::nextafterf(p, 0.f)); in.push_back(p); in.push_back(std::nextafterf(p, INFINITY));
    }
    int n = 0;
    for (int top : {10, 12})
        for (float mx : in) {
            // the rule written out: mx = f 2^e with f in [0.5, 1) -> 2^(top - e); 2^0 where mx has no exponent to take
            int e = 0;
            if (mx > 0.f && std::isfinite(mx)) { (void)std::frexp(mx, &e); e = top - e; }
            const float want = std::ldexp(1.0f, e);
            const float got = pow2_scale(mx, top);
            CHECK(same_bits(got, want), "pow2_scale(%a, %d) = %a, formula %a", mx, top, got, want);
            // Finite positive normal input is scaled into [2^(top - 1), 2^top) - wherever fp32 can hold the scale: 2^(top - e) needs
            // top - e <= 127, that is mx >= 2^(top - 128).  Below that (FLT_MIN and the denormals: a weight tensor that is zero to
            // fp16 at any scale) no fp32 factor can do it and the rule, as every copy of it did, returns +inf; the equality above
            // pins that down
            if (std::isnormal(mx) && mx >= std::ldexp(1.0f, top - 128)) {
                const float v = mx * got;   // exact: a power-of-two factor, result far from fp32's limits
                CHECK(v >= std::ldexp(1.0f, top - 1) && v < std::ldexp(1.0f, top), "pow2_scale(%a, %d): scaled %a outside [2^%d, 2^%d)", mx, top, v, top - 1, top);
            }
            if (!(mx > 0.f) || !std::isfinite(mx)) CHECK(same_bits(got, 1.0f), "pow2_scale(%a, %d) = %a, expected 1", mx, top, got);
            ++n;
        }
    std::printf("pow2_scale: %d inputs\n", n);
}

// range_exponent (range_exponent.h): the exponent of a DYNAMIC operand's planes, the one function the kernels (strip_common.h) and the
// host entries that write planes for them (capi.hip: ace_dhconv_strip_op) share.  Inside its clamp it is pow2_scale(mx, 12)'s exponent;
// beyond it the two part by a power of two - which is what ace_dhconv_f16x3 got wrong while it scaled with pow2_scale and the
// kernel unscaled with the clamped exponent (max |coeffs| = 2^-95: e = 106 against 100; 2^115: -104 against -100).
static void check_range_exponent() {
    std::vector<float> in = {0.f, -1.f, std::numeric_limits<float>::denorm_min(), FLT_MIN, 2.9e38f, 3.0e38f, FLT_MAX, INFINITY, NAN};
    for (int k : {-120, -95, -90, -89, -88, -20, 0, 11, 12, 30, 111, 112, 113, 115, 120}) {
        const float p = std::ldexp(1.0f, k);
        in.push_back(std::nextafterf(p, 0.f)); in.push_back(p); in.push_back(std::nextafterf(p, INFINITY));
    }
    int n = 0, nclamped = 0;
    for (float mx : in) {
        bool clamped = true;
        const int e = range_exponent(mx, &clamped);
        CHECK(e == range_exponent(mx), "range_exponent(%a) depends on the flag", mx);
        CHECK(e >= -100 && e <= 100, "range_exponent(%a) = %d", mx, e);
        if (!(mx > 0.f) || !(mx < 3.0e38f)) { CHECK(e == 0 && !clamped, "range_exponent(%a) = %d, expected 0", mx, e); ++n; continue; }
        int f = 0;
        (void)std::frexp(mx, &f);
        const int raw = 12 - f;
        CHECK(e == (raw > 100 ? 100 : raw < -100 ? -100 : raw) && clamped == (raw != e), "range_exponent(%a) = %d (clamped %d), 12 - exponent = %d", mx, e, (int)clamped, raw);
        if (!clamped) {   // the planes hold mx in [2^11, 2^12), and the static rule agrees bit for bit
            const float v = mx * std::ldexp(1.0f, e);
            CHECK(v >= 2048.f && v < 4096.f, "range_exponent(%a): scaled %a", mx, v);
            CHECK(same_bits(std::ldexp(1.0f, e), pow2_scale(mx, 12)), "range_exponent(%a) and pow2_scale(.., 12) differ inside the clamp", mx);
            CHECK(mx >= std::ldexp(1.0f, -89) && mx < std::ldexp(1.0f, 112), "unclamped outside [2^-89, 2^112): %a", mx);
        } else {          // ... outside they differ: the host must not take pow2_scale there
            CHECK(!same_bits(std::ldexp(1.0f, e), pow2_scale(mx, 12)), "range_exponent(%a): clamped, yet equal to pow2_scale", mx);
            CHECK(mx < std::ldexp(1.0f, -89) || mx >= std::ldexp(1.0f, 112), "clamped inside [2^-89, 2^112): %a", mx);
            ++nclamped;
        }
        ++n;
    }
    CHECK(range_exponent(std::ldexp(1.0f, -95)) == 100 && range_exponent(std::ldexp(1.0f, 115)) == -100, "the two ends the operator test runs");
    CHECK(nclamped >= 10, "only %d clamped inputs", nclamped);
    std::printf("range_exponent: %d inputs, %d beyond the clamp\n", n, nclamped);
}

static void check_weight_norms() {
    const int shapes[4][3] = {{1, 1, 1}, {3, 5, 5}, {16, 33, 64}, {128, 384, 384}};   // rows, cols, ld
    std::mt19937 rng(20240611);
    std::normal_distribution<float> nd(0.f, 1.f);
    for (const auto& sh : shapes) {
        const int rows = sh[0], cols = sh[1], ld = sh[2];
        std::vector<float> w((size_t)rows * ld, NAN);   // padding columns: NaN - a read of one would poison either norm
        float mx = 0.f;
        long double rmax = 0.0L;
        for (int r = 0; r < rows; ++r) {
            long double rs = 0.0L;
            for (int c = 0; c < cols; ++c) {
                const float v = nd(rng) * std::ldexp(1.0f, (int)(rng() % 9) - 4);
                w[(size_t)r * ld + c] = v;
                mx = std::fmax(mx, std::fabs(v));
                rs += std::fabs((long double)v);
            }
            rmax = rs > rmax ? rs : rmax;
        }
        const WeightNorms nm = weight_norms(w.data(), rows, cols, ld);
        CHECK(same_bits(nm.absmax, mx), "%d x %d / %d: absmax %a, expected %a", rows, cols, ld, nm.absmax, mx);
        // winf = fl32(rowsum_fp64 (1 + 1e-6)): the fp64 sum of <= 384 terms is off by < 1e-13 relative, the inflation lifts it by 1e-6
        // and the rounding to fp32 moves it by at most 2^-24 = 6e-8 - never below the true sum, never past (1 + 2e-6) of it
        CHECK((long double)nm.winf >= rmax, "%d x %d / %d: winf %.9g below the row-sum maximum %.9Lg", rows, cols, ld, nm.winf, rmax);
        CHECK((long double)nm.winf <= rmax * (1.0L + 2e-6L), "%d x %d / %d: winf %.9g above (1 + 2e-6) x %.9Lg", rows, cols, ld, nm.winf, rmax);
        std::printf("weight_norms %3d x %3d / %3d: absmax %.6g  winf / rowsum - 1 = %.3Lg\n", rows, cols, ld, nm.absmax, (long double)nm.winf / rmax - 1.0L);
    }
}

// "does the handle need the per-sample fold buffer of fc1 (Wq1)?", as ace_sfno_create asks it: for any block of the net
static bool needs_wq1(int num_layers, long hw_data, long hw_inner, int ws_roles, bool wl_on, int C, int hid) {
    return any_block(num_layers, hw_data, hw_inner,
                     [&](long hw) { return fc1_on_conv_ws(ws_roles, C, hid, hw) || fc1_on_conv_wl(wl_on, C, hid, hw); });
}

static void check_storage_question() {
    const int C = 384, hid = 768;
    {   // 180 x 360, scale_factor 1, every role on: what is eligible today stays eligible
        const long hw = 180L * 360;
        CHECK(skip_on_conv_ws(7, C, C, hw), "skip");
        CHECK(fc1_on_conv_ws(7, C, hid, hw), "fc1 on conv_ws");
        CHECK(fc1_on_conv_wl(true, C, hid, hw), "fc1 on conv_wl");
        CHECK(fc2_on_conv_ws(7, hid, C, hw), "fc2");
        CHECK(fc2_on_conv_ws(7, C, C, hw), "last encoder convolution");
        CHECK(cln_skip_on_conv_ws(7, C, C, hw), "cln skip");
        CHECK(needs_wq1(8, hw, hw, 7, true, C, hid), "Wq1 at the headline shape");
        CHECK(!fc1_on_conv_wl(false, C, hid, hw) && !skip_on_conv_ws(6, C, C, hw) && !fc1_on_conv_ws(5, C, hid, hw) && !fc2_on_conv_ws(3, hid, C, hw) &&
                  !cln_skip_on_conv_ws(6, C, C, hw), "switched-off roles stay off");
    }
    {   // 721 x 1440, scale_factor 2, conv_wl off: fc1 (K = 384 -> M = 768) on conv_ws.hip.  The kernel addresses its fp32-sized output
        // rows with 32-bit byte offsets, M HW 4 < 0x7fffff00 = 2 147 483 392:
        //   data grid   721 x 1440 = 1 038 240 pixels: 768 x 1 038 240 x 4 = 3 189 473 280  -> past the limit, not eligible
        //   inner grid  360 x  720 =   259 200 pixels: 768 x   259 200 x 4 =   796 262 400  -> fits; statistics (259 200 / 32 + 8) x 768 x 16
        //                                                                  =    99 631 104  -> fits, eligible
        // so blocks 0 .. n - 2 (which run on the inner grid) take conv_ws.hip and the handle needs Wq1, although the data grid says no
        const long hw_data = 721L * 1440, hw_inner = 360L * 720;
        CHECK(!fc1_on_conv_ws(7, C, hid, hw_data), "fc1 on conv_ws at the data grid");
        CHECK(fc1_on_conv_ws(7, C, hid, hw_inner), "fc1 on conv_ws at the inner grid");
        CHECK(needs_wq1(8, hw_data, hw_inner, 7, false, C, hid), "Wq1 for any block");
        CHECK(!needs_wq1(1, hw_data, hw_inner, 7, false, C, hid), "a one-block net of that shape runs on the data grid only");
    }
    {   // the grid a block's skips and MLP run on
        const long hw_data = 48L * 96, hw_inner = 24L * 48;
        CHECK(block_out_pixels(0, 1, hw_data, hw_inner) == hw_data, "one-block net: data grid");
        CHECK(block_out_pixels(0, 3, hw_data, hw_inner) == hw_inner, "block 0 of 3: inner grid");
        CHECK(block_out_pixels(1, 3, hw_data, hw_inner) == hw_inner, "block 1 of 3: inner grid");
        CHECK(block_out_pixels(2, 3, hw_data, hw_inner) == hw_data, "last block of 3: data grid");
    }
    std::printf("storage question: done\n");
}

int main() {
    check_pow2_scale();
    check_range_exponent();
    check_weight_norms();
    check_storage_question();
    if (bad) { std::printf("%d checks FAILED\n", bad); return 1; }
    std::printf("weight prep ok\n");
    return 0;
}
