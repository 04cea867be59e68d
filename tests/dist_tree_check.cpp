// dist_tree_check.cpp -- stand-alone CPU check of csrc/rt_dist_tree.h (tests/test_distance_cpu.py builds and runs it;
// no HIP).  usage: dist_tree_check <in> <out>
//   in : u32 nt, u32 np, f32 tris[nt][3][3], f32 points[np][3]
//   out: u32 levels (the blocks + the upper levels), u32 order[nt], then per level (0 = the blocks):
//        u32 n, f32 bound[n][np] -- the kernel's cull bound lb(node box) - margin of every (node, point), formed by
//        the operations of rt_distance.hip's node_needed (one f32 rounding each, no contraction)
// The program itself checks, and exits 1 with a message on the first failure:
//   * order is a permutation of [0, nt); the blocks' first Morton codes ascend;
//   * level counts: n_0 = ceil(nt / 32), n_(j+1) = ceil(n_j / 32), the top level holds at most 32 nodes and every
//     level below it more than 32 -- so the nodes' record ranges [i 32^(j+1), (i+1) 32^(j+1)) partition [0, nt);
//   * every block box is EXACTLY the min / max of its records' vertices; every upper box exactly that of its children
//     (hence every box holds its triangles' vertices and every parent holds its children);
//   * bound(parent, p) <= bound(child, p) for every point: the float box distance is monotone.
// The caller compares the bounds with the oracle's distances.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../cpp-11-ray-trace-march-framework_amd/csrc/rt_dist_tree.h"

#define FAIL(...)                      \
    do {                               \
        std::fprintf(stderr, __VA_ARGS__); \
        std::fprintf(stderr, "\n");    \
        return 1;                      \
    } while (0)

static float bound(const float *box, const float *p, float scale)
{
    const float margin = 1e-5f * (std::fmax(std::fmax(std::fabs(p[0]), std::fabs(p[1])), std::fabs(p[2])) + scale);
    float e[3];
    for (int a = 0; a < 3; a++) e[a] = std::fmax(std::fmax(box[a] - p[a], p[a] - box[4 + a]), 0.0f);
    const float s = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
    return std::sqrt(s) - margin;
}

int main(int argc, char **argv)
{
    if (argc != 3) FAIL("usage: dist_tree_check <in> <out>");
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) FAIL("cannot open %s", argv[1]);
    uint32_t hdr[2];
    if (std::fread(hdr, 4, 2, f) != 2) FAIL("short header");
    const uint32_t nt = hdr[0], np = hdr[1];
    std::vector<float> tris(size_t(nt) * 9), pts(size_t(np) * 3);
    if (std::fread(tris.data(), 4, tris.size(), f) != tris.size() || std::fread(pts.data(), 4, pts.size(), f) != pts.size())
        FAIL("short input");
    std::fclose(f);
    std::vector<uint32_t> idx(size_t(nt) * 3);
    for (size_t i = 0; i < idx.size(); i++) idx[i] = uint32_t(i);

    rtk::DistTree T;
    rtk::dist_tree_build(tris.data(), 3, nt * 3, idx.data(), 3, nt, T);

    // the order is a permutation; the keys ascend
    if (T.order.size() != nt) FAIL("order has %zu entries for %u triangles", T.order.size(), nt);
    std::vector<char> seen(nt, 0);
    for (uint32_t k = 0; k < nt; k++)
    {
        if (T.order[k] >= nt || seen[T.order[k]]) FAIL("order[%u] = %u is out of range or repeated", k, T.order[k]);
        seen[T.order[k]] = 1;
    }
    if (T.nblk != (nt + 31) / 32 || T.blk.size() != size_t(T.nblk) * 8 || T.blk_key.size() != T.nblk)
        FAIL("%u blocks for %u triangles", T.nblk, nt);
    for (uint32_t b = 1; b < T.nblk; b++)
        if (T.blk_key[b] < T.blk_key[b - 1]) FAIL("block keys descend at %u", b);
    for (uint32_t b = 0; b < T.nblk; b++)
        if (T.blk_key[b] >> rtk::kDistKeyBits) FAIL("block key %u wider than %u bits", b, rtk::kDistKeyBits);
    // the level counts
    if (T.nlevels > rtk::kDistMaxLevels) FAIL("%u upper levels", T.nlevels);
    {
        uint32_t n = T.nblk;
        size_t off = 0;
        for (uint32_t l = 0; l < T.nlevels; l++)
        {
            if (n <= rtk::kDistFan) FAIL("level %u built over %u nodes", l + 1, n);
            n = (n + rtk::kDistFan - 1) / rtk::kDistFan;
            if (T.lvl_n[l] != n || T.lvl_off[l] != off) FAIL("level %u: n %u off %u, want %u %zu", l + 1, T.lvl_n[l], T.lvl_off[l], n, off);
            off += n;
        }
        if (n > rtk::kDistFan) FAIL("top level holds %u nodes", n);
        if (T.nodes.size() != off * 8) FAIL("nodes holds %zu floats, want %zu", T.nodes.size(), off * 8);
    }
    // block boxes: exactly their records' vertices
    for (uint32_t b = 0; b < T.nblk; b++)
    {
        float mn[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, mx[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
        for (uint32_t k = b * 32; k < std::min(nt, b * 32 + 32); k++)
            for (int v = 0; v < 3; v++)
                for (int a = 0; a < 3; a++)
                {
                    const float c = tris[size_t(T.order[k]) * 9 + v * 3 + a];
                    mn[a] = std::min(mn[a], c);
                    mx[a] = std::max(mx[a], c);
                }
        for (int a = 0; a < 3; a++)
            if (T.blk[size_t(b) * 8 + a] != mn[a] || T.blk[size_t(b) * 8 + 4 + a] != mx[a]) FAIL("block %u: box is not exact", b);
    }
    // upper boxes: exactly their children's; bounds monotone
    std::vector<std::vector<float>> bounds(T.nlevels + 1);
    for (uint32_t l = 0; l <= T.nlevels; l++)
    {
        const float *box = l == 0 ? T.blk.data() : T.nodes.data() + size_t(T.lvl_off[l - 1]) * 8;
        const uint32_t n = l == 0 ? T.nblk : T.lvl_n[l - 1];
        bounds[l].resize(size_t(n) * np);
        for (uint32_t i = 0; i < n; i++)
            for (uint32_t p = 0; p < np; p++) bounds[l][size_t(i) * np + p] = bound(box + size_t(i) * 8, &pts[size_t(p) * 3], T.scale);
        if (l == 0) continue;
        const float *cbox = l == 1 ? T.blk.data() : T.nodes.data() + size_t(T.lvl_off[l - 2]) * 8;
        const uint32_t nc = l == 1 ? T.nblk : T.lvl_n[l - 2];
        for (uint32_t i = 0; i < n; i++)
        {
            float mn[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, mx[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
            for (uint32_t c = i * 32; c < std::min(nc, i * 32 + 32); c++)
            {
                for (int a = 0; a < 3; a++)
                {
                    mn[a] = std::min(mn[a], cbox[size_t(c) * 8 + a]);
                    mx[a] = std::max(mx[a], cbox[size_t(c) * 8 + 4 + a]);
                }
                for (uint32_t p = 0; p < np; p++)
                    if (bounds[l][size_t(i) * np + p] > bounds[l - 1][size_t(c) * np + p])
                        FAIL("level %u node %u point %u: the parent's bound exceeds child %u's", l, i, p, c);
            }
            for (int a = 0; a < 3; a++)
                if (box[size_t(i) * 8 + a] != mn[a] || box[size_t(i) * 8 + 4 + a] != mx[a]) FAIL("level %u node %u: box is not exact", l, i);
        }
    }
    f = std::fopen(argv[2], "wb");
    if (!f) FAIL("cannot open %s", argv[2]);
    const uint32_t levels = T.nlevels + 1;
    std::fwrite(&levels, 4, 1, f);
    std::fwrite(T.order.data(), 4, nt, f);
    for (uint32_t l = 0; l < levels; l++)
    {
        const uint32_t n = l == 0 ? T.nblk : T.lvl_n[l - 1];
        std::fwrite(&n, 4, 1, f);
        std::fwrite(bounds[l].data(), 4, bounds[l].size(), f);
    }
    std::fclose(f);
    std::printf("nt %u: %u blocks, %u upper levels, top %u\n", nt, T.nblk, T.nlevels, T.nlevels ? T.lvl_n[T.nlevels - 1] : T.nblk);
    return 0;
}
