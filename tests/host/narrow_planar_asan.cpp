// Narrow planar storage (vbc.h VBC_CREATE_NARROW_PLANAR) in the planner, as a program of its own for an
// AddressSanitizer / UBSan build of the create path's host code (make plan_asan PLAN_ASAN_SRC=<this file>).
// narrow_planar_asan CASE IMAGE_180 IMAGE_80: reads the case file of tests/host/plan_asan.cpp (the flags in it
// without the two narrow bits; val: Float32 values widened to Float64), plans it with VBC_CREATE_NARROW_VALUES |
// VBC_CREATE_NARROW_PLANAR and with VBC_CREATE_NARROW_VALUES alone under the knobs of the environment, and
// writes the two arena images.  It also checks that VBC_CREATE_NARROW_PLANAR alone is refused.  Exit status 0
// when all of that went as expected.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "vbc.h"
#include "vbc_host.h"

template <typename T>
static std::vector<T> take(FILE *f, int64_t n)
{
    std::vector<T> v((size_t)n);
    if (n > 0 && fread(v.data(), sizeof(T), (size_t)n, f) != (size_t)n) v.clear();
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int64_t> h = take<int64_t>(f, 11);
    const std::vector<vbcx_facts> facts = take<vbcx_facts>(f, 1);
    if (h.size() != 11 || facts.empty() || h[10] != 8) return 2;
    const int64_t m = h[0], n = h[1], U = h[2], W = h[3], K = h[4], L = h[5], q = h[6], nval = h[7];
    const std::vector<int64_t> pspl = take<int64_t>(f, K > 0 ? K + 1 : 0), spl = take<int64_t>(f, L + 1),
                               pos = take<int64_t>(f, L + 1), idx = take<int64_t>(f, q), ofs = take<int64_t>(f, L + 1);
    const std::vector<char> val = take<char>(f, nval * 8);
    fclose(f);
    const unsigned base = (unsigned)h[9] & ~(VBC_CREATE_NARROW_VALUES | VBC_CREATE_NARROW_PLANAR);
    auto plan = [&](unsigned flags, std::vector<char> &img) {
        size_t bytes = 0;
        img.clear();
        for (int pass = 0; pass < 2; pass++) {  // the size, then the image
            const int st = vbcx_plan_image(m, n, U, W, K, K > 0 ? pspl.data() : nullptr, L, spl.data(), pos.data(),
                                           idx.data(), ofs.data(), val.data(), nval, (int)h[8], flags, facts.data(),
                                           pass ? img.data() : nullptr, img.size(), &bytes);
            if (st != VBC_OK) return st;
            img.resize(bytes);
        }
        return (int)VBC_OK;
    };
    std::vector<char> img;
    if (plan(base | VBC_CREATE_NARROW_PLANAR, img) != VBC_INVALID_ARG) {
        fprintf(stderr, "%s: VBC_CREATE_NARROW_PLANAR alone was not refused\n", argv[1]);
        return 1;
    }
    const unsigned both = VBC_CREATE_NARROW_VALUES | VBC_CREATE_NARROW_PLANAR;
    for (int k = 0; k < 2; k++) {
        const int st = plan(base | (k ? VBC_CREATE_NARROW_VALUES : both), img);
        if (st != VBC_OK) {
            char msg[512];
            vbc_last_error(msg, sizeof msg);
            fprintf(stderr, "%s: status %d: %s\n", argv[1], st, msg);
            return 1;
        }
        f = fopen(argv[2 + k], "wb");
        if (!f || fwrite(img.data(), 1, img.size(), f) != img.size()) return 2;
        fclose(f);
    }
    return 0;
}
