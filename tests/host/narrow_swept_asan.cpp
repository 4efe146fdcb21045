// Narrow row-swept storage (vbc.h VBC_CREATE_NARROW_SWEPT) in the planner, as a program of its own for an
// AddressSanitizer / UBSan build of the create path's host code (make plan_asan PLAN_ASAN_SRC=<this file>).
// narrow_swept_asan CASE IMAGE_1080 MAP CHUNKS: reads the case file of tests/host/plan_asan.cpp (the flags in it
// without the narrow bits; val: Float32 values widened to Float64) and, under the knobs of the environment
// (VBC_SWEEP=1 lays every bucket of width <= 8 out swept), plans it with 0x1080 (VBC_CREATE_NARROW_VALUES |
// VBC_CREATE_NARROW_SWEPT) and with 0x1280 (the same with VBC_CREATE_NARROW_UPDATABLE, which must give the same
// image), then asks for the value map of the 0x1280 handle (the two recording plans, whose swept writer copies tags
// into the narrow regions).  It writes the image, the map and the chunk table, and checks that 0x1000 without 0x80
// is refused whatever other narrow bits come with it.  Exit status 0 when all of that went as expected.
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

template <typename T>
static bool put(const char *path, const std::vector<T> &v)
{
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
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
    const unsigned v80 = VBC_CREATE_NARROW_VALUES, p100 = VBC_CREATE_NARROW_PLANAR, p400 = VBC_CREATE_NARROW_PAIRS,
                   s800 = VBC_CREATE_NARROW_STREAMS, w1000 = VBC_CREATE_NARROW_SWEPT;
    const unsigned n1080 = v80 | w1000;
    const unsigned base = (unsigned)h[9] & ~(v80 | p100 | p400 | s800 | w1000 | VBC_CREATE_NARROW_UPDATABLE);
    auto report = [&](int st) {
        char msg[512];
        vbc_last_error(msg, sizeof msg);
        fprintf(stderr, "%s: status %d: %s\n", argv[1], st, msg);
    };
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
    std::vector<char> img, img2;
    for (unsigned part : {0u, p100, p400, p100 | p400, p100 | p400 | s800}) {
        if (plan(base | w1000 | part, img) != VBC_INVALID_ARG) {
            fprintf(stderr, "%s: VBC_CREATE_NARROW_SWEPT with 0x%x and without 0x80 was not refused\n", argv[1], part);
            return 1;
        }
    }
    if (int st = plan(base | n1080, img)) { report(st); return 1; }
    if (int st = plan(base | n1080 | VBC_CREATE_NARROW_UPDATABLE, img2)) { report(st); return 1; }
    if (img != img2) {
        fprintf(stderr, "%s: the 0x1280 image differs from the 0x1080 image\n", argv[1]);
        return 1;
    }
    auto ask = [&](uint32_t *map, int64_t mcap, int64_t *ne, vbcx_map_chunk *ch, int64_t ccap, int64_t *nc) {
        const int st = vbcx_value_map(m, n, U, W, K, K > 0 ? pspl.data() : nullptr, L, spl.data(), pos.data(), idx.data(),
                                      ofs.data(), val.data(), nval, (int)h[8], base | n1080 | VBC_CREATE_NARROW_UPDATABLE,
                                      facts.data(), map, mcap, ne, ch, ccap, nc);
        if (st != VBC_OK) report(st);
        return st;
    };
    int64_t ne = 0, nc = 0, ne2 = 0, nc2 = 0;
    if (ask(nullptr, 0, &ne, nullptr, 0, &nc) != VBC_OK || ne < 1 || nc < 1) return 1;
    // exactly as large as the counts: a write past either end is the sanitizer's to report
    std::vector<uint32_t> map((size_t)ne);
    std::vector<vbcx_map_chunk> chunks((size_t)nc);
    if (ask(map.data(), ne, &ne2, chunks.data(), nc, &nc2) != VBC_OK || ne2 != ne || nc2 != nc) return 1;
    if (!put(argv[2], img) || !put(argv[3], map) || !put(argv[4], chunks)) return 2;
    return 0;
}
