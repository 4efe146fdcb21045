// The layout planner as a program of its own, for an AddressSanitizer / UBSan build of the create path's host
// code (make plan_asan).  plan_asan CASE IMAGE: plans the case that tests/test_plan_host.py wrote to CASE -- 11
// Int64 (m, n, U, W, K, L, stored blocks, nval, dtype, flags, bytes per value), the facts (vbcx_facts), then
// pspl (K + 1 entries when K > 0), spl, pos, idx, ofs and val -- through vbcx_plan_image, under the knobs of the
// environment, and writes the arena image to IMAGE.  Exit status 0 when the plan succeeds.
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
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int64_t> h = take<int64_t>(f, 11);
    const std::vector<vbcx_facts> facts = take<vbcx_facts>(f, 1);
    if (h.size() != 11 || facts.empty()) return 2;
    const int64_t m = h[0], n = h[1], U = h[2], W = h[3], K = h[4], L = h[5], q = h[6], nval = h[7];
    const std::vector<int64_t> pspl = take<int64_t>(f, K > 0 ? K + 1 : 0), spl = take<int64_t>(f, L + 1),
                               pos = take<int64_t>(f, L + 1), idx = take<int64_t>(f, q), ofs = take<int64_t>(f, L + 1);
    const std::vector<char> val = take<char>(f, nval * h[10]);
    fclose(f);
    size_t bytes = 0;
    std::vector<char> img;
    for (int pass = 0; pass < 2; pass++) {  // the size, then the image
        const int st = vbcx_plan_image(m, n, U, W, K, K > 0 ? pspl.data() : nullptr, L, spl.data(), pos.data(), idx.data(),
                                       ofs.data(), val.data(), nval, (int)h[8], (unsigned)h[9], facts.data(),
                                       pass ? img.data() : nullptr, img.size(), &bytes);
        if (st != VBC_OK) {
            char msg[512];
            vbc_last_error(msg, sizeof msg);
            fprintf(stderr, "%s: status %d: %s\n", argv[1], st, msg);
            return 1;
        }
        img.resize(bytes);
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(img.data(), 1, img.size(), f) != img.size()) return 2;
    fclose(f);
    return 0;
}
