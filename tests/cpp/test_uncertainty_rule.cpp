// The pure-host parts of the measurement uncertainty (putslam_amd/csrc/ps_uncertainty_rule.h) in a plain C++ program: the sensor
// model's defaults, the table of the colour gradient's ties -- the same at every magnitude, every entry -1, 0 or 1, the packed form
// gives every entry back --, and the argument rule, case by case.  tests/test_uncertainty_ref_host.py builds it with
// -fsanitize=address,undefined and runs it on the CPU: no GPU, no HIP.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ps_uncertainty_rule.h"

static int failures = 0;
#define CHECK(cond)                                                 \
    do {                                                            \
        if (!(cond)) {                                              \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                             \
        }                                                           \
    } while (0)

int main()
{
    // the defaults (depthSensorModel.h:53-58); the scale factors are 0
    PsSensorModel s;
    std::memset(&s, 0xA5, sizeof s);
    unc_sensor_default(s);
    CHECK(s.fu == 582.64 && s.fv == 586.97 && s.cu == 320.17 && s.cv == 260.0 && s.varU == 1.1046 && s.varV == 0.64160);
    CHECK(s.c3 == -8.9997e-06 && s.c2 == 3.069e-003 && s.c1 == 3.6512e-006 && s.c0 == -0.0017512e-3);
    CHECK(s.scaleUncertaintyNormal == 0.0 && s.scaleUncertaintyGradient == 0.0);
    CHECK(sizeof(PsSensorModel) == 96);

    // the ties: one table for every magnitude, up to the largest gradient there is
    int32_t one[20], other[20];
    unc_tie_table(1, one);
    const int ks[] = {1, 2, 3, 7, 1000, 12345, 16 * 65535};
    for (int k : ks) {
        unc_tie_table(k, other);
        CHECK(std::memcmp(one, other, sizeof one) == 0);
    }
    for (int k = 0; k < 20; ++k) CHECK(one[k] >= -1 && one[k] <= 1);
    const unsigned long long w = unc_tie_pack(one);
    for (int k = 0; k < 20; ++k) CHECK(unc_tie_entry(w, k) == one[k]);
    CHECK((w >> 40) == 0);
    std::printf("ties:");
    for (int k = 0; k < 20; ++k) std::printf(" %d", one[k]);
    std::printf("\n");

    // the argument rule
    std::vector<uint16_t> dpix(3 * 14 * 24);
    std::vector<uint8_t> ipix(3 * 14 * 64);
    PsFrameGeometry g{};
    PsDepthSet d{};
    d.pixels = dpix.data(), d.rowStride = 48, d.frameStride = 0, d.numFrames = 3, d.rows = 14, d.cols = 20;
    PsImageSet im{};
    im.pixels = ipix.data(), im.rowStride = 64, im.frameStride = 0, im.numFrames = 3, im.rows = 14, im.cols = 20, im.channels = 3;
    UncStrides st;
    const char *why = nullptr;
    CHECK(unc_sets_error(&g, &s, 2, &im, &d, true, true, st, why) == PS_OK);
    CHECK(st.dRow == 48 && st.dFrame == 14 * 48 && st.iRow == 64 && st.iFrame == 14 * 64);
    CHECK(unc_sets_error(&g, nullptr, -1, nullptr, &d, false, false, st, why) == PS_OK && st.iRow == 0 && st.dRow == 48);
    CHECK(unc_sets_error(nullptr, &s, 0, &im, &d, false, true, st, why) == PS_ERR_BAD_ARG && why);
    CHECK(unc_sets_error(&g, nullptr, 0, &im, &d, false, true, st, why) == PS_ERR_BAD_ARG);
    CHECK(unc_sets_error(&g, &s, 0, &im, nullptr, false, true, st, why) == PS_ERR_BAD_ARG);
    CHECK(unc_sets_error(&g, &s, 3, &im, &d, false, true, st, why) == PS_ERR_BAD_ARG);
    CHECK(unc_sets_error(&g, &s, -2, &im, &d, false, true, st, why) == PS_ERR_BAD_ARG);
    CHECK(unc_sets_error(&g, &s, 2, nullptr, &d, true, true, st, why) == PS_ERR_BAD_ARG);
    for (int cn : {1, 2, 4}) {
        PsImageSet grey = im;
        grey.channels = cn;
        CHECK(unc_sets_error(&g, &s, 0, &grey, &d, false, true, st, why) == PS_ERR_UNSUPPORTED);
    }
    {
        PsDepthSet b = d;
        b.rowStride = 38;
        CHECK(unc_sets_error(&g, &s, 0, nullptr, &b, false, true, st, why) == PS_ERR_BAD_ARG);
        b = d, b.rowStride = 41;
        CHECK(unc_sets_error(&g, &s, 0, nullptr, &b, false, true, st, why) == PS_ERR_BAD_ARG);
        b = d, b.frameStride = 13 * 48 + 38;
        CHECK(unc_sets_error(&g, &s, 0, nullptr, &b, false, true, st, why) == PS_ERR_BAD_ARG);
        b = d, b.frameStride = 13 * 48 + 40;
        CHECK(unc_sets_error(&g, &s, 0, nullptr, &b, false, true, st, why) == PS_OK && st.dFrame == 13 * 48 + 40);
        b = d, b.numFrames = -1;
        CHECK(unc_sets_error(&g, &s, 0, nullptr, &b, false, true, st, why) == PS_ERR_BAD_ARG);
        b = d, b.pixels = nullptr;
        CHECK(unc_sets_error(&g, &s, 0, nullptr, &b, false, true, st, why) == PS_ERR_BAD_ARG);
        b.numFrames = 0;
        CHECK(unc_sets_error(&g, &s, 0, nullptr, &b, false, true, st, why) == PS_OK);
        b = d, b.rows = 0;
        CHECK(unc_sets_error(&g, &s, 0, nullptr, &b, false, true, st, why) == PS_ERR_BAD_ARG);
    }
    {
        PsImageSet b = im;
        b.rowStride = 59;
        CHECK(unc_sets_error(&g, &s, 2, &b, &d, true, true, st, why) == PS_ERR_BAD_ARG);
        b = im, b.frameStride = 13 * 64 + 59;
        CHECK(unc_sets_error(&g, &s, 2, &b, &d, true, true, st, why) == PS_ERR_BAD_ARG);
        b = im, b.rows = 13;
        CHECK(unc_sets_error(&g, &s, 2, &b, &d, true, true, st, why) == PS_ERR_BAD_ARG);
        b = im, b.cols = 21;
        CHECK(unc_sets_error(&g, &s, 2, &b, &d, true, true, st, why) == PS_ERR_BAD_ARG);
        b = im, b.pixels = nullptr;
        CHECK(unc_sets_error(&g, &s, 2, &b, &d, true, true, st, why) == PS_ERR_BAD_ARG);
        b = im, b.numFrames = -3;
        CHECK(unc_sets_error(&g, &s, 2, &b, &d, true, true, st, why) == PS_ERR_BAD_ARG);
    }
    if (failures) return 1;
    std::printf("uncertainty rule ok\n");
    return 0;
}
