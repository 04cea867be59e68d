// rt_dist_tree.h -- the distance kernels' scene data: the Morton order of the triangles, its
// blocks of kDistTreeBlock records with exact float boxes and first Morton codes, and the box hierarchy over the
// blocks.  Host only, no HIP, C++11: rt_scene_create (rt_tracer.hip) runs dist_tree_build and
// tests/dist_tree_check.cpp checks the same function on the CPU.
//
// Level 0 is the blocks.  Level j >= 1 groups kDistFan consecutive nodes of level j - 1 into one node whose box
// is the componentwise min / max of theirs; levels are added until the top one holds at most kDistFan nodes.  One
// upper level covers 1,024 triangles per node, two cover 32,768; a mesh of 2^20 triangles has a top level of
// exactly 32 nodes, and no mesh of fewer than 2^32 triangles needs more than kDistMaxLevels upper levels.
// Node i of level j covers the sorted records [i * 32^(j+1), min(nt, (i + 1) * 32^(j+1))): the ranges of a level
// partition [0, nt), and a parent's range is the union of its children's.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace rtk {

constexpr uint32_t kDistTreeBlock = 32;     // records per block (= kDistBlock, rt_kparams.h)
constexpr uint32_t kDistFan = 32;           // children per node
constexpr uint32_t kDistMaxLevels = 5;      // upper levels: 2^27 blocks / 32^5 = 4 top nodes
constexpr uint32_t kDistKeyBits = 30;       // Morton code: 10 bits an axis

struct DistTree
{
    std::vector<uint32_t> order;        // [nt] sorted record -> mesh triangle
    std::vector<uint32_t> blk_key;      // [nblk] Morton code of every block's first record (ascending)
    std::vector<float> blk;             // [nblk][2][4] {min.xyz, 0} {max.xyz, 0}
    std::vector<float> nodes;           // the upper levels back to back, same layout
    uint32_t nblk = 0, nlevels = 0;     // nlevels: upper levels (0: the blocks are the top)
    uint32_t lvl_off[kDistMaxLevels] = { 0, 0, 0, 0, 0 };   // first node of upper level j + 1 in `nodes`
    uint32_t lvl_n[kDistMaxLevels] = { 0, 0, 0, 0, 0 };     // its node count
    float vmin[3] = { 0, 0, 0 }, vmax[3] = { 0, 0, 0 };     // the vertex box
    float scale = 0.0f;                 // max |vertex coordinate|
};

// 10 bits an axis, x the highest of each triple (the order rt_scene_create has always sorted by)
inline uint32_t dist_morton(const uint32_t q[3])
{
    uint32_t code = 0;
    for (int bit = 9; bit >= 0; bit--)
        for (int a = 0; a < 3; a++) code = (code << 1) | ((q[a] >> bit) & 1u);
    return code;
}

// verts: vertex v's position at verts[v * vstride .. + 2]; tris: triangle t's vertex indices at
// tris[t * tstride .. + 2] (rt_vertex / rt_triangle: both strides 6)
inline void dist_tree_build(const float *verts, size_t vstride, uint32_t nv, const uint32_t *tris, size_t tstride,
                            uint32_t nt, DistTree& T)
{
    float mn[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, mx[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
    float scale = 0.0f;
    for (uint32_t i = 0; i < nv; i++)
        for (int a = 0; a < 3; a++)
        {
            const float c = verts[i * vstride + a];
            mn[a] = std::min(mn[a], c);
            mx[a] = std::max(mx[a], c);
            scale = std::max(scale, c < 0.0f ? -c : c);
        }
    for (int a = 0; a < 3; a++)
    {
        T.vmin[a] = mn[a];
        T.vmax[a] = mx[a];
    }
    T.scale = scale;
    // Morton order of the centroids (ties: ascending triangle index)
    std::vector<std::pair<uint64_t, uint32_t>> order(nt);
    for (uint32_t i = 0; i < nt; i++)
    {
        const uint32_t *t = tris + i * tstride;
        uint32_t q[3];
        for (int a = 0; a < 3; a++)
        {
            const double c = (double(verts[t[0] * vstride + a]) + verts[t[1] * vstride + a] + verts[t[2] * vstride + a]) / 3.0;
            const double ext = double(mx[a]) - double(mn[a]);
            const double f = ext > 0.0 ? (c - mn[a]) / ext : 0.0;
            q[a] = uint32_t(std::min(1023.0, std::max(0.0, f * 1024.0)));
        }
        order[i] = { uint64_t(dist_morton(q)), i };
    }
    std::sort(order.begin(), order.end());
    T.order.resize(nt);
    for (uint32_t k = 0; k < nt; k++) T.order[k] = order[k].second;
    // level 0: the blocks
    T.nblk = (nt + kDistTreeBlock - 1) / kDistTreeBlock;
    T.blk.assign(size_t(T.nblk) * 8, 0.0f);
    T.blk_key.resize(T.nblk);
    for (uint32_t b = 0; b < T.nblk; b++)
    {
        float bmn[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, bmx[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
        for (uint32_t k = b * kDistTreeBlock; k < std::min(nt, (b + 1) * kDistTreeBlock); k++)
        {
            const uint32_t *t = tris + order[k].second * tstride;
            for (int v = 0; v < 3; v++)
                for (int a = 0; a < 3; a++)
                {
                    const float c = verts[t[v] * vstride + a];
                    bmn[a] = std::min(bmn[a], c);
                    bmx[a] = std::max(bmx[a], c);
                }
        }
        for (int a = 0; a < 3; a++)
        {
            T.blk[size_t(b) * 8 + a] = bmn[a];
            T.blk[size_t(b) * 8 + 4 + a] = bmx[a];
        }
        T.blk_key[b] = uint32_t(order[size_t(b) * kDistTreeBlock].first);
    }
    // the upper levels
    T.nlevels = 0;
    T.nodes.clear();
    const float *child = T.blk.data();
    uint32_t nchild = T.nblk;
    size_t child_off = 0;               // the children's first node in T.nodes (upper levels only)
    bool child_upper = false;
    while (nchild > kDistFan && T.nlevels < kDistMaxLevels)
    {
        const uint32_t n = (nchild + kDistFan - 1) / kDistFan;
        const size_t off = T.nodes.size() / 8;
        T.nodes.resize((off + n) * 8, 0.0f);
        if (child_upper) child = T.nodes.data() + child_off * 8;       // (resize may have moved the array)
        for (uint32_t i = 0; i < n; i++)
        {
            float *o = T.nodes.data() + (off + i) * 8;
            for (int a = 0; a < 3; a++)
            {
                o[a] = FLT_MAX;
                o[4 + a] = -FLT_MAX;
            }
            for (uint32_t c = i * kDistFan; c < std::min(nchild, (i + 1) * kDistFan); c++)
                for (int a = 0; a < 3; a++)
                {
                    o[a] = std::min(o[a], child[size_t(c) * 8 + a]);
                    o[4 + a] = std::max(o[4 + a], child[size_t(c) * 8 + 4 + a]);
                }
        }
        T.lvl_off[T.nlevels] = uint32_t(off);
        T.lvl_n[T.nlevels] = n;
        T.nlevels++;
        child_off = off;
        child_upper = true;
        child = T.nodes.data() + off * 8;
        nchild = n;
    }
}

} // namespace rtk
