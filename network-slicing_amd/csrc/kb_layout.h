// kb_layout.h -- how a KBRL dictionary lies in its pool, and the work line every agent transfer walks.  Plain C++: nothing
// from HIP, so that a host compiler reads it too (tests/test_kb_layout.py walks it under the address and UB sanitizers).
//
// A dictionary is a run of shells of 64 landmarks (kb_kbrl.hip, "Storage"); shell b is its vector page and, by KbDev.tri,
//     1            [ page ][ lower tiles (b,0) .. (b,b) ][ (b + 1) x 128 partial sums ]     one agent per replica
//     0            [ page ][ lower tiles (b,0) .. (b,b) ][ upper tiles (0,b) .. (b-1,b) ]    shared dictionaries
//     KB_TRI_NONE  [ page ]                                                                inference only: no Kinv
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KB_HD __host__ __device__
#else
#define KB_HD
#endif

#define KB_CH 64          // landmarks per chunk
#define KB_TILE 4096      // doubles per Kinv tile
#define KB_VEC_ROWS 30
#define KB_VEC (KB_VEC_ROWS * KB_CH)
#define KB_TRI_NONE 2     // KbDev.tri of an inference-only handle
#define KB_FORK_BLK 2048  // doubles (16 KB) of the destination pool one wave copies per turn

namespace kb {

KB_HD inline uint64_t kb_shell_doubles(int b, int tri) {  // tri 1: b + 1 tiles and their 128 partial sums each
    if (tri == KB_TRI_NONE) return (uint64_t)KB_VEC;
    return (uint64_t)KB_VEC + (tri ? (uint64_t)(b + 1) * (KB_TILE + 128) : (uint64_t)(2 * b + 1) * KB_TILE);
}
// doubles of the shells 0 .. b - 1 of one dictionary: where shell b starts in a dictionary laid out whole.  b pages and, of
// tiles, 1 + 2 + .. + b with their partial sums (tri 1), 1 + 3 + .. + (2 b - 1) = b^2 (tri 0), none (KB_TRI_NONE)
KB_HD inline uint64_t kb_shells_before(int b, int tri) {
    const uint64_t n = (uint64_t)b;
    const uint64_t tile = tri == KB_TRI_NONE ? 0 : tri ? KB_TILE + 128 : KB_TILE, tiles = tri ? n * (n + 1) / 2 : n * n;
    return n * KB_VEC + tile * tiles;
}
// the part of shell b that is the same bytes in both storages that hold Kinv: the vector page and the lower tiles
KB_HD inline uint64_t kb_shell_common(int b) { return (uint64_t)KB_VEC + (uint64_t)(b + 1) * KB_TILE; }

// ---- the work line.  Dictionaries laid out whole, one behind the other, fill [64, top) of a pool without a gap: base[0 .. n]
// is the scan of their sizes from 64 (offset 0 means "no shell"), base[n] = top.  The line is that range cut into pieces of
// KB_FORK_BLK doubles, a wave each: balanced by bytes whatever the dictionaries' sizes.
KB_HD inline uint64_t kb_line_pieces(uint64_t top) { return (top - 64 + KB_FORK_BLK - 1) / KB_FORK_BLK; }

// the last dictionary that starts at or before p (empty ones share their start with the next)
KB_HD inline int kb_line_find(const uint64_t* base, int n, uint64_t p) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (base[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Piece `blk` of the line, run by run: the piece finds its dictionary by bisection of the scan and its shell by walking the
// sizes of storage `tri`; a run ends with the piece or where cut(b, in, sz) -- an offset in shell b of sz doubles, beyond `in`
// -- says it does inside the shell.  body(jd, b, in, p, seg): seg doubles from pool position p, which is offset `in` of shell b
// of dictionary jd.  Every size and every cut is a multiple of 64 doubles, so every run is, and is 16-byte aligned.
template <class Cut, class Body>
KB_HD inline void kb_line_walk(const uint64_t* base, int n, int tri, uint64_t blk, Cut cut, Body body) {
    const uint64_t top = base[n];
    uint64_t p = 64 + blk * KB_FORK_BLK;
    const uint64_t pe = p + KB_FORK_BLK < top ? p + KB_FORK_BLK : top;
    int jd = kb_line_find(base, n, p);
    while (p < pe) {
        while (base[jd + 1] <= p) ++jd;  // (p < top = base[n]: ends)
        const uint64_t q = p - base[jd];
        int b = 0;
        uint64_t c = 0, sz = kb_shell_doubles(0, tri);
        while (q >= c + sz) {
            c += sz;
            ++b;
            sz = kb_shell_doubles(b, tri);
        }
        const uint64_t in = q - c, end = cut(b, in, sz);
        const uint64_t seg = end - in < pe - p ? end - in : pe - p;
        body(jd, b, in, p, seg);
        p += seg;
    }
}

// the cuts: where a run that stands at offset `in` of shell b ends
struct KbCutShell {  // the whole shell
    KB_HD uint64_t operator()(int, uint64_t, uint64_t sz) const { return sz; }
};
struct KbCutPage {  // the vector page, then the rest
    KB_HD uint64_t operator()(int, uint64_t in, uint64_t sz) const { return in < KB_VEC ? (uint64_t)KB_VEC : sz; }
};
struct KbCutCommon {  // the part common to both storages, then the rest (tri 1: the partial-sum area)
    KB_HD uint64_t operator()(int b, uint64_t in, uint64_t sz) const { return in < kb_shell_common(b) ? kb_shell_common(b) : sz; }
};
struct KbCutTiles {  // the common part, then tile by tile (tri 0: the upper tiles) up to the shell's end
    KB_HD uint64_t operator()(int b, uint64_t in, uint64_t sz) const {
        const uint64_t common = kb_shell_common(b);
        if (in < common) return common;
        const uint64_t end = common + ((in - common) / KB_TILE + 1) * KB_TILE;
        return end < sz ? end : sz;
    }
};

}  // namespace kb
