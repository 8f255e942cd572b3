// The scaffold of the stand-alone sanitizer programs of the query definitions (tests/{box_query,tri_query,hull_query,nearest,nearest_multi,
// multi_hit}_sanitize.cpp): the CHECK that counts failures, a small tree over given rows, and for the three overlap queries the check of one output
// slot.  Each program includes it as "query_sanitize.hpp", which finds it next to the including file, and keeps its own query makers, its main and
// the exact array lengths it allocates.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++g_fail; } } while (0)

struct Tree { std::vector<float> nodes, tris; int nNodes = 0, nTris = 0; };

// rows of tris12 from tris9 (v0, e1, e2), and a median split by index over them with leaves of at most 8: any tree over the rows serves here
static void grow(Tree &T, int first, int count) {
    const int me = T.nNodes++;
    T.nodes.resize((size_t)T.nNodes * 12, 0.0f);
    float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
    for (int i = first; i < first + count; ++i) {
        const float *t = &T.tris[(size_t)i * 12];
        for (int a = 0; a < 3; ++a)
            for (float v : {t[a], t[a] + t[4 + a], t[a] + t[8 + a]}) { lo[a] = std::min(lo[a], v); hi[a] = std::max(hi[a], v); }
    }
    for (int a = 0; a < 3; ++a) { T.nodes[(size_t)me * 12 + a] = lo[a]; T.nodes[(size_t)me * 12 + 4 + a] = hi[a]; }
    if (count <= 8) { T.nodes[(size_t)me * 12 + 8] = (float)first; T.nodes[(size_t)me * 12 + 9] = (float)count; return; }
    const int half = count / 2;
    const int l = T.nNodes;
    grow(T, first, half);
    const int r = T.nNodes;
    grow(T, first + half, count - half);
    T.nodes[(size_t)me * 12 + 3] = (float)l; T.nodes[(size_t)me * 12 + 7] = (float)r;
}
static Tree tree_of(const std::vector<float> &tris9) {
    Tree T;
    T.nTris = (int)tris9.size() / 9;
    T.tris.assign((size_t)T.nTris * 12, 0.0f);
    for (int i = 0; i < T.nTris; ++i)
        for (int k = 0; k < 3; ++k) std::memcpy(&T.tris[(size_t)i * 12 + 4 * k], &tris9[(size_t)i * 9 + 3 * k], 12);
    grow(T, 0, T.nTris);
    return T;
}

// What one call of an overlap query leaves of a slot: the count within [0, nTris]; the first min(room, count) entries distinct rows of the tree; the
// rest untouched
static inline void check_slot(const Tree &T, const int32_t *slot, int64_t room, int32_t count, int32_t mark) {
    CHECK(count >= 0 && count <= T.nTris);
    const int64_t kept = std::min<int64_t>(std::max<int64_t>(room, 0), count);
    for (int64_t j = 0; j < kept; ++j) {
        CHECK(slot[j] >= 0 && slot[j] < T.nTris);
        for (int64_t k = 0; k < j; ++k) CHECK(slot[k] != slot[j]);
    }
    for (int64_t j = kept; j < room; ++j) CHECK(slot[j] == mark);
}
