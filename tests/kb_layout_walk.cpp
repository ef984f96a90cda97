// The work-line walker and the layout arithmetic of csrc/kb_layout.h on the host, built with the address and undefined-behaviour
// sanitizers and run by tests/test_kb_layout.py.  Dictionaries of 0, 0, 1, 64, 65, 0, 128, 200, 257, 0, 63, 320 and 0 landmarks
// (empty ones at the start, in the middle and at the end; 257 and 320 landmarks are 5 shells) are laid out in each of the three
// storages; every piece of the line is walked under every cut that applies, and every run is held to what the kernels rely on.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kb_layout.h"

using namespace kb;

static const int kM[] = {0, 0, 1, 64, 65, 0, 128, 200, 257, 0, 63, 320, 0};
static const int kN = (int)(sizeof kM / sizeof kM[0]);

#define CHECK(cond, ...)                                         \
    do {                                                         \
        if (!(cond)) {                                           \
            std::fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                   \
            std::fprintf(stderr, "\n");                          \
            std::exit(1);                                        \
        }                                                        \
    } while (0)

enum { CUT_SHELL, CUT_PAGE, CUT_COMMON, CUT_TILES };
static const char* kCutName[] = {"whole shell", "page / rest", "common / partial sums", "common / tile by tile"};

// the offsets inside shell b that a run of the cut must not cross, stated apart from the functors under test
static std::vector<uint64_t> boundaries(int cut, int b, int tri) {
    std::vector<uint64_t> at;
    const uint64_t sz = kb_shell_doubles(b, tri), common = (uint64_t)KB_VEC + (uint64_t)(b + 1) * KB_TILE;
    if (cut == CUT_PAGE) at.push_back(KB_VEC);
    if (cut == CUT_COMMON || cut == CUT_TILES) at.push_back(common);
    if (cut == CUT_TILES)
        for (uint64_t x = common + KB_TILE; x < sz; x += KB_TILE) at.push_back(x);
    at.push_back(sz);
    return at;
}

template <class Cut>
static long walk(int tri, int cut_kind, Cut cut) {
    std::vector<uint64_t> base((size_t)kN + 1);
    uint64_t top = 64;
    for (int j = 0; j < kN; ++j) {
        base[(size_t)j] = top;
        top += kb_shells_before((kM[j] + KB_CH - 1) / KB_CH, tri);
    }
    base[(size_t)kN] = top;
    std::vector<unsigned char> seen((size_t)top, 0);
    long runs = 0;
    const uint64_t pieces = kb_line_pieces(top);
    for (uint64_t blk = 0; blk < pieces; ++blk) {
        kb_line_walk(base.data(), kN, tri, blk, cut, [&](int jd, int b, uint64_t in, uint64_t p, uint64_t seg) {
            ++runs;
            CHECK(jd >= 0 && jd < kN, "dictionary %d", jd);
            CHECK(b >= 0 && b < (kM[jd] + KB_CH - 1) / KB_CH, "shell %d of dictionary %d of %d landmarks", b, jd, kM[jd]);
            CHECK(seg > 0 && seg % 64 == 0, "run of %llu doubles", (unsigned long long)seg);
            CHECK(p == base[(size_t)jd] + kb_shells_before(b, tri) + in, "p %llu, dictionary %d shell %d offset %llu", (unsigned long long)p,
                  jd, b, (unsigned long long)in);
            CHECK(p >= 64 + blk * KB_FORK_BLK && p + seg <= 64 + (blk + 1) * KB_FORK_BLK && p + seg <= top, "run [%llu, %llu) of piece %llu",
                  (unsigned long long)p, (unsigned long long)(p + seg), (unsigned long long)blk);
            for (uint64_t x : boundaries(cut_kind, b, tri))
                CHECK(!(in < x && x < in + seg), "run [%llu, %llu) of shell %d crosses %llu", (unsigned long long)in,
                      (unsigned long long)(in + seg), b, (unsigned long long)x);
            CHECK(in + seg <= kb_shell_doubles(b, tri), "run ends at %llu of shell %d", (unsigned long long)(in + seg), b);
            for (uint64_t q = p; q < p + seg; ++q) {
                CHECK(!seen[(size_t)q], "double %llu lies in two runs", (unsigned long long)q);
                seen[(size_t)q] = 1;
            }
        });
    }
    for (uint64_t q = 64; q < top; ++q) CHECK(seen[(size_t)q], "double %llu lies in no run", (unsigned long long)q);
    std::printf("storage %d, %s: %llu doubles, %llu pieces, %ld runs\n", tri, kCutName[cut_kind], (unsigned long long)(top - 64),
                (unsigned long long)pieces, runs);
    return runs;
}

int main() {
    const int storages[] = {0, 1, KB_TRI_NONE};
    for (int tri : storages) {
        uint64_t sum = 0;
        for (int b = 0; b <= 16; ++b) {
            CHECK(kb_shells_before(b, tri) == sum, "kb_shells_before(%d, %d) = %llu, the shells' sizes add up to %llu", b, tri,
                  (unsigned long long)kb_shells_before(b, tri), (unsigned long long)sum);
            sum += kb_shell_doubles(b, tri);
        }
    }
    long runs = 0;
    for (int tri : storages) {
        runs += walk(tri, CUT_SHELL, KbCutShell());
        runs += walk(tri, CUT_PAGE, KbCutPage());
        if (tri == KB_TRI_NONE) continue;  // (the other two cuts are of storages that hold tiles)
        runs += walk(tri, CUT_COMMON, KbCutCommon());
        runs += walk(tri, CUT_TILES, KbCutTiles());
    }
    std::printf("%ld runs\n", runs);
    return 0;
}
