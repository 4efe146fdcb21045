// The value map of an updatable handle (vbc_host.h vbcx_value_map: the two recording plans and the comparison of
// their images, narrow value regions included) as a program of its own for an AddressSanitizer / UBSan build of the
// create path's host code (make plan_asan PLAN_ASAN_SRC=<this file>).
// value_map_asan CASE MAP CHUNKS: reads the case file of tests/host/plan_asan.cpp (flags with the narrow bits; val:
// Float32 values widened to Float64), asks for the counts, then for the map and the chunk table under the knobs of
// the environment, and writes both.  It also checks that a buffer too small for the count is left alone.  Exit
// status 0 when all of that went as expected.
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
    auto ask = [&](uint32_t *map, int64_t mcap, int64_t *ne, vbcx_map_chunk *ch, int64_t ccap, int64_t *nc) {
        const int st = vbcx_value_map(m, n, U, W, K, K > 0 ? pspl.data() : nullptr, L, spl.data(), pos.data(), idx.data(),
                                      ofs.data(), val.data(), nval, (int)h[8], (unsigned)h[9], facts.data(), map, mcap, ne,
                                      ch, ccap, nc);
        if (st != VBC_OK) {
            char msg[512];
            vbc_last_error(msg, sizeof msg);
            fprintf(stderr, "%s: status %d: %s\n", argv[1], st, msg);
        }
        return st;
    };
    int64_t ne = 0, nc = 0;
    if (ask(nullptr, 0, &ne, nullptr, 0, &nc) != VBC_OK) return 1;
    if (ne < 1 || nc < 1) return 1;
    // exactly as large as the counts: a write past either end is the sanitizer's to report
    std::vector<uint32_t> map((size_t)ne);
    std::vector<vbcx_map_chunk> chunks((size_t)nc);
    uint32_t one = 7;
    int64_t ne2 = 0, nc2 = 0;
    if (ask(&one, 1, &ne2, nullptr, 0, &nc2) != VBC_OK || (ne > 1 && one != 7) || ne2 != ne || nc2 != nc) return 1;
    if (ask(map.data(), ne, &ne2, chunks.data(), nc, &nc2) != VBC_OK || ne2 != ne || nc2 != nc) return 1;
    f = fopen(argv[2], "wb");
    if (!f || fwrite(map.data(), 4, map.size(), f) != map.size()) return 2;
    fclose(f);
    f = fopen(argv[3], "wb");
    if (!f || fwrite(chunks.data(), sizeof(vbcx_map_chunk), chunks.size(), f) != chunks.size()) return 2;
    fclose(f);
    return 0;
}
