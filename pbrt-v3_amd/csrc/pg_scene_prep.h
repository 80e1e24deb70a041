// pg_scene_prep.h -- everything pg_scene_create (pg_abi.hip) does with the caller's PgSceneDesc before it touches the device:
// the checks of the description and the host-side layout of what the kernels read.  Host code only: no HIP runtime call, so
// a program without a device can run it (tests/scene_prep_host.hip does, under the sanitizers).  pg_prepare_scene is a sequence
// of stages; each does its checks, then its layout, in the order the checks have always been reached.
#ifndef PG_SCENE_PREP_H
#define PG_SCENE_PREP_H
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "pg_device.h"
#include "pg_kernels.h"
// An array the caller already holds in the device's layout: uploaded verbatim, never copied on the host.
struct HostSpan { const void *p = nullptr; size_t bytes = 0; void set(const void *q, size_t n) { p = q; bytes = n; } };
struct PreparedScene {
    DScene d;  // scalars and flags only; every pointer still null
    int nt = 0, nnAll = 0;  // primitives / nodes, those of object definitions included
    // arrays built here
    std::vector<float4> wnodes, tris, triS, lightHot;
    std::vector<DObject> objects;
    std::vector<DInstEntry> instEntry;
    std::vector<float> uv, triAttr;       // (uv: kept only for scenes with alpha-masked meshes, DScene::alphaUV)
    std::vector<PgMaterial> materials;    // a plastic's roughness already remapped
    std::vector<int32_t> primes, haltonDims;
    std::vector<DAlphaTex> alphaTex;
    std::vector<float> bxdfsPk, distTable;  // (distTable: the uniform / power light distribution)
    std::vector<int2> matPk;
    std::vector<unsigned char> primClass;
    // arrays of the description that are uploaded as they are
    HostSpan nodes, instances, spheres, bxdfs, textures, textured, images, texels, ewaLut, envTables, lights, perms, permSums, cmaxmin, alphas, triAlpha,
        bssrdfs, materialBssrdf, bssrdfTables, media, triMediumIn, triMediumOut, grids, mediaGrid, gridDensity, noisePerm, sobolMatrices, vdcSobol, vdcSobolInv;
    // what pg_scene_create keeps in PgScene
    int matStride = 0, nMedia = 0;
    bool volOrder = false, hasNullMaterial = false;
    // the "spatial" light distribution: a dense table of denseVoxels distributions computed on the device, or (DScene::sparseLights)
    // nVoxelsTotal voxels computed on first touch into a pool of poolSlots; distStride floats per distribution
    size_t denseVoxels = 0, distStride = 0;
    int nVoxelsTotal = 0, poolSlots = 0;
    bool anyLobeMaterial = false, anyImageLight = false;  // (between the stages)
};
inline int pgPrepFail(std::string &err, int code, const char *fmt, ...) {
    char buf[1024];
    va_list a;
    va_start(a, fmt);
    vsnprintf(buf, sizeof(buf), fmt, a);
    va_end(a);
    err = buf;
    return code;
}
#define PREP_FAIL(code, ...) return pgPrepFail(err, code, __VA_ARGS__)
#define PREP_STAGE(call) do { int st_ = (call); if (st_ != PG_OK) return st_; } while (0)

// --- child-pair records for k_trace (pg_traverse.hip): one 64-B record per interior node
struct PgRecordBuilder {
    const PgSceneDesc *desc;
    std::vector<float4> &w;
    int leafBits;
    int recordLayout;  // which records share a 128-B line (measured, profiles/r03n_record_layout_ab.txt: 1 is 1 - 3 % faster than 0, 2 is no gain)
    bool badChildren = false;
    int worldPending = 0, objectPending = 0;  // stack entries the world BVH / the deepest object BVH can have pending
    // The node array comes from the caller: before anything is indexed by it, require the reference's layout
    // (bvh.cpp:640-658: first child at i + 1, second child later in the array) and that it is a tree -- every node but
    // the root the child of exactly one interior node -- so that every interior node is reached from the root once.
    // The same pass takes the greatest number of entries a traversal can have pending, which the stack must hold.
    void checkTree(const PgBVHNode *nodes, int nn, bool world) {
        std::vector<int> level((size_t)nn, 0);
        std::vector<unsigned char> parents((size_t)nn, 0);
        int deepest = 0;
        for (int i = 0; i < nn && !badChildren; ++i) {
            if (i > 0 && parents[i] != 1) { badChildren = true; break; }
            if (nodes[i].nprims != 0) continue;
            const int c0 = i + 1;
            const long long c1 = nodes[i].offset;
            if (c0 >= nn || c1 <= c0 || c1 >= nn || parents[c0] || parents[c1] || nodes[i].axis > 2) { badChildren = true; break; }
            parents[c0] = parents[c1] = 1;
            level[c0] = level[c1] = level[i] + 1;  // entries pending while a child of node i is visited: <= level
            deepest = std::max(deepest, level[i] + 1);
        }
        if (!badChildren) (world ? worldPending : objectPending) = std::max(world ? worldPending : objectPending, deepest);
    }
    // Two records share a 128-B line, and an L2 miss fills the whole line: choose the line mates.  1: a node with the
    // child a ray through it is likelier to visit (the one with the larger surface area); 2: the two children of a
    // node.  Nodes left alone (no interior child / sibling) pair up among themselves in the order they are met.
    // Returns the number of interior nodes that got a slot.
    int placeLineMates(const PgBVHNode *nodes, int nn, int base, std::vector<int> &recIndex) const {
        auto area = [&](int i) { const PgBVHNode &b = nodes[i]; const float x = b.bmax[0] - b.bmin[0], y = b.bmax[1] - b.bmin[1], z = b.bmax[2] - b.bmin[2]; return x * y + y * z + z * x; };
        int nPlaced = 0;  // (base is even: lines are pairs of absolute record indices, and nodes are placed two at a time)
        auto place = [&](int n) { recIndex[n] = base + nPlaced++; };
        std::vector<int> singles, stack;
        if (nn > 0 && nodes[0].nprims == 0) stack.push_back(0);
        auto placeSingle = [&](int n) { singles.push_back(n); if (singles.size() == 2) { place(singles[0]); place(singles[1]); singles.clear(); } };
        while (!stack.empty()) {
            const int n = stack.back(); stack.pop_back();
            const int c0 = n + 1, c1 = nodes[n].offset;
            if (c0 >= nn || c1 <= n || c1 >= nn) continue;  // (reported by buildRecords)
            const bool i0 = nodes[c0].nprims == 0, i1 = nodes[c1].nprims == 0;
            if (recordLayout == 1) {  // `n` is the head of a line unless it was placed as its parent's mate
                int h = -1, o = -1;
                if (i0 && i1) { h = area(c0) >= area(c1) ? c0 : c1; o = h == c0 ? c1 : c0; } else if (i0) h = c0; else if (i1) h = c1;
                if (recIndex[n] < 0) {
                    if (h < 0) { placeSingle(n); continue; }
                    place(n); place(h);
                    if (o >= 0) stack.push_back(o);
                    // h's own children head new lines
                    const int h0 = h + 1, h1 = nodes[h].offset;
                    if (h1 > h && h1 < nn && h0 < nn) { if (nodes[h1].nprims == 0) stack.push_back(h1); if (nodes[h0].nprims == 0) stack.push_back(h0); }
                }
            } else {  // siblings share a line
                if (n == 0) placeSingle(n);  // (the root; every other node is placed, or waits among the singles, when it is pushed)
                if (i0 && i1) { place(c0); place(c1); stack.push_back(c1); stack.push_back(c0); }
                else if (i0) { placeSingle(c0); stack.push_back(c0); }
                else if (i1) { placeSingle(c1); stack.push_back(c1); }
            }
        }
        if (singles.size() == 1) place(singles[0]);
        return nPlaced;
    }
    // one BVHAccel's nodes [firstNode, +nn) -> records appended to w; leaf references carry GLOBAL primitive indices
    // (firstPrim + the node's own offset).  Returns the reference of the BVH's root.
    int buildRecords(int firstNode, int nn, int firstPrim) {
        const PgBVHNode *nodes = desc->nodes + firstNode;
        checkTree(nodes, nn, firstNode == 0);
        if (badChildren) return TR_NO_ROOT;
        std::vector<int> recIndex((size_t)nn, -1);
        int nInterior = 0;
        if (recordLayout != 0 && ((w.size() / 4) & 1)) w.resize(w.size() + 4, make_float4(0, 0, 0, 0));
        const int base = (int)(w.size() / 4);
        for (int i = 0; i < nn; ++i) if (nodes[i].nprims == 0) ++nInterior;
        if (recordLayout == 0) {  // depth-first: a record's line mate is the next interior node of the reference's array
            int k = 0;
            for (int i = 0; i < nn; ++i) if (nodes[i].nprims == 0) recIndex[i] = base + k++;
        } else if (placeLineMates(nodes, nn, base, recIndex) != nInterior) badChildren = true;  // every interior node has exactly one slot
        auto refOf = [&](int i) -> int {
            const PgBVHNode &nd = nodes[i];
            return nd.nprims == 0 ? recIndex[i] : ~(((firstPrim + nd.offset) << leafBits) | (nd.nprims - 1));
        };
        w.resize((size_t)(base + nInterior) * 4);
        for (int i = 0; i < nn; ++i) {
            const PgBVHNode &nd = nodes[i];
            if (nd.nprims != 0) continue;
            const int c0 = i + 1, c1 = nd.offset;
            if (c0 >= nn || c1 <= i || c1 >= nn) { badChildren = true; continue; }
            const PgBVHNode &a = nodes[c0], &b = nodes[c1];
            float4 *r = &w[(size_t)recIndex[i] * 4];
            r[0] = make_float4(a.bmin[0], a.bmax[0], b.bmin[0], b.bmax[0]);
            r[1] = make_float4(a.bmin[1], a.bmax[1], b.bmin[1], b.bmax[1]);
            r[2] = make_float4(a.bmin[2], a.bmax[2], b.bmin[2], b.bmax[2]);
            int r0 = refOf(c0), r1 = refOf(c1), ax = nd.axis;
            float f0, f1, f2;
            memcpy(&f0, &r0, 4); memcpy(&f1, &r1, 4); memcpy(&f2, &ax, 4);
            r[3] = make_float4(f0, f1, f2, 0.f);
        }
        return nn > 0 ? refOf(0) : TR_NO_ROOT;
    }
};
// TransformedPrimitives: their instances exist, and those inside object definitions nest one level only
inline int pgPrepCheckInstances(const PgSceneDesc *desc, int traceDepth, int worldPending, int objectPending, PreparedScene &ps, std::string &err) {
    DScene &d = ps.d;
    const int nt = ps.nt;
    for (int k = 0; k < nt; ++k) {
        const uint32_t f = desc->tri_flags ? desc->tri_flags[k] : 0;
        if (!(f & PG_PRIM_INSTANCE)) continue;
        const int ii = desc->indices[3 * k];
        if (ii < 0 || ii >= desc->n_instances || !desc->instances || desc->instances[ii].object < 0 || desc->instances[ii].object >= desc->n_objects)
            PREP_FAIL(PG_ERR_INVALID, "primitive %d: instance %d / its object out of range", k, ii);
        if (k >= desc->n_tris) {
            // ABI 29: a TransformedPrimitive among an object definition's primitives (a moving shape inside ObjectBegin / ObjectEnd, api.cpp:1386-1419):
            // ONE level -- what it wraps holds shapes only, as in the reference, whose ObjectInstance cannot appear inside a definition (api.cpp:1549-1552)
            const PgObject &inner = desc->objects[desc->instances[ii].object];
            for (int q = inner.first_prim; q < inner.first_prim + inner.n_prims; ++q)
                if (q < 0 || q >= nt || (desc->tri_flags[q] & PG_PRIM_INSTANCE))
                    PREP_FAIL(PG_ERR_UNSUPPORTED, "primitive %d: a TransformedPrimitive inside an object definition wraps another one (more than two levels)", k);
            if (k >= inner.first_prim && k < inner.first_prim + inner.n_prims) PREP_FAIL(PG_ERR_INVALID, "primitive %d: an object definition contains itself", k);
            d.hasNest = 1;
        }
    }
    if (d.hasNest) {
        // hitInst = outer + n_instances * (inner + 1) in an int; three BVHs share k_trace's stack
        if ((int64_t)desc->n_instances * ((int64_t)desc->n_instances + 1) >= ((int64_t)1 << 31))
            PREP_FAIL(PG_ERR_UNSUPPORTED, "%d instances in a scene with TransformedPrimitives inside object definitions: the pair (outer, inner) does not fit a hit's instance word", desc->n_instances);
        if (worldPending + 2 * objectPending > TR_STACK_TOTAL + traceDepth)
            PREP_FAIL(PG_ERR_UNSUPPORTED, "world BVH (%d levels) + two object BVHs (%d levels) exceed the traversal stack of %d entries", worldPending, objectPending, TR_STACK_TOTAL + traceDepth);
    }
    return PG_OK;
}
// --- BVH records, object definitions, instances
inline int pgPrepBvh(const PgSceneDesc *desc, int traceDepth, PreparedScene &ps, std::string &err) {
    DScene &d = ps.d;
    const int nt = ps.nt, nnAll = ps.nnAll;
    ps.nodes.set(desc->nodes, sizeof(PgBVHNode) * (size_t)nnAll);  // uploaded verbatim (32 B/node, same bytes as pbrt's LinearBVHNode)
    int maxLeaf = 1;
    for (int i = 0; i < nnAll; ++i) if (desc->nodes[i].nprims > maxLeaf) maxLeaf = desc->nodes[i].nprims;
    int leafBits = 0;
    while ((1 << leafBits) < maxLeaf) ++leafBits;
    if ((uint64_t)nt >= ((uint64_t)1 << (31 - leafBits)) - 1)
        PREP_FAIL(PG_ERR_UNSUPPORTED, "%d triangles with up to %d per leaf exceed the 31-bit leaf reference", nt, maxLeaf);
    PgRecordBuilder rb{desc, ps.wnodes, leafBits, getenv("PG_RECORD_LAYOUT") ? atoi(getenv("PG_RECORD_LAYOUT")) : 1};
    const int nn = desc->n_nodes;
    const int topRef = rb.buildRecords(0, nn, 0);
    // object definitions (instancing): each with its own records, root box and root reference
    if (desc->n_objects > 0 && !desc->objects) PREP_FAIL(PG_ERR_INVALID, "pg_scene_create: n_objects = %d without an objects array", desc->n_objects);
    std::vector<DObject> &objs = ps.objects;
    objs.resize((size_t)(desc->n_objects > 0 ? desc->n_objects : 0));
    for (size_t k = 0; k < objs.size(); ++k) {
        const PgObject &o = desc->objects[k];
        if (o.first_prim < desc->n_tris || o.n_prims < 1 || o.first_prim + o.n_prims > nt || o.n_nodes < 0 ||
            (o.n_nodes > 0 && (o.first_node < desc->n_nodes || o.first_node + o.n_nodes > nnAll)) || (o.n_nodes == 0 && o.n_prims != 1))
            PREP_FAIL(PG_ERR_INVALID, "object %d: nodes [%d, +%d) / primitives [%d, +%d) out of range", (int)k, o.first_node, o.n_nodes, o.first_prim, o.n_prims);
        DObject &dobj = objs[k];
        memset(&dobj, 0, sizeof(dobj));
        dobj.firstPrim = o.first_prim;
        dobj.nNodes = o.n_nodes;
        if (o.n_nodes > 0) {
            dobj.rootRef = rb.buildRecords(o.first_node, o.n_nodes, o.first_prim);
            for (int c = 0; c < 3; ++c) { dobj.box[c] = desc->nodes[o.first_node].bmin[c]; dobj.box[3 + c] = desc->nodes[o.first_node].bmax[c]; }
        }
    }
    if (rb.badChildren) PREP_FAIL(PG_ERR_INVALID, "the BVH node array is not a tree in the reference's layout (a child out of range, shared or unreachable)");
    // k_trace's stack (csrc/pg_traverse.hip): TR_STACK_TOTAL entries behind the LDS part, shared by the world traversal and the
    // instance traversal above it; the reference-order any-hit kernel keeps one bit per pending entry of ONE tree in a 64-bit
    // mask.  The reference itself has int nodesToVisit[64] per BVH (bvh.cpp:670, :708) and no check at all.
    const int worldPending = rb.worldPending, objectPending = rb.objectPending;
    if (worldPending > TR_STACK_TOTAL || objectPending > TR_STACK_TOTAL)
        PREP_FAIL(PG_ERR_UNSUPPORTED, "a BVH is %d levels deep: more than the 64 pending nodes of the reference's traversal stack (bvh.cpp:670)",
                  std::max(worldPending, objectPending));
    if (worldPending + objectPending > TR_STACK_TOTAL + traceDepth)
        PREP_FAIL(PG_ERR_UNSUPPORTED, "world BVH (%d levels) + object BVH (%d levels) exceed the traversal stack of %d entries", worldPending, objectPending,
                  TR_STACK_TOTAL + traceDepth);
    PREP_STAGE(pgPrepCheckInstances(desc, traceDepth, worldPending, objectPending, ps, err));
    if (desc->n_instances > 0 && desc->instances) { ps.instances.set(desc->instances, sizeof(PgInstance) * (size_t)desc->n_instances); d.nInstances = desc->n_instances; }
    if (d.nInstances > 0 && !objs.empty()) {
        ps.instEntry.resize((size_t)desc->n_instances);
        for (int i = 0; i < desc->n_instances; ++i) {
            const PgInstance &in = desc->instances[i];
            DInstEntry &e = ps.instEntry[i];
            memset(&e, 0, sizeof(e));
            if (in.object < 0 || in.object >= desc->n_objects) continue;  // (never referenced: the primitives' instances were checked above)
            const DObject &ob = objs[in.object];
            memcpy(e.w2i, in.w2i, sizeof(e.w2i));
            memcpy(e.box, ob.box, sizeof(e.box));
            e.rootRef = ob.rootRef; e.firstPrim = ob.firstPrim; e.nNodes = ob.nNodes;
            const float last[4] = {0.f, 0.f, 0.f, 1.f};
            e.affineStill = (!in.animated && memcmp(in.w2i + 12, last, sizeof(last)) == 0) ? 1 : 0;  // (bitwise: -0 is not 0 here)
        }
    }
    for (int i = 0; i < d.nInstances; ++i) if (desc->instances[i].animated) d.hasMotion = d.rayTimes = 1;
    d.leafBits = leafBits;
    if (nn > 0) d.rootRef = topRef;
    for (int k = 0; k < 3 && nn > 0; ++k) { d.rootBox[k] = desc->nodes[0].bmin[k]; d.rootBox[3 + k] = desc->nodes[0].bmax[k]; }
    return PG_OK;
}
// the record of a primitive that is no triangle: tris[k] = (index, 0, 0, flags), (0, 0, 0, material), (0, 0, 0, light)
inline void pgPrepIndexRecord(float4 *t, int index, uint32_t flags, int mat, int light) {
    float iw, fw, mw, lw;
    memcpy(&iw, &index, 4); memcpy(&fw, &flags, 4); memcpy(&mw, &mat, 4); memcpy(&lw, &light, 4);
    t[0] = make_float4(iw, 0, 0, fw);
    t[1] = make_float4(0, 0, 0, mw);
    t[2] = make_float4(0, 0, 0, lw);
}
// --- primitives and their attributes.  Triangles: vertices gathered into BVH order, 48 B per triangle
inline int pgPrepPrimitives(const PgSceneDesc *desc, PreparedScene &ps, std::string &err) {
    const int nt = ps.nt;
    std::vector<float4> &tris = ps.tris;
    std::vector<float> &uv = ps.uv;
    tris.assign((size_t)nt * PG_TRI_STRIDE, make_float4(0, 0, 0, 0));
    bool anyUV = false;
    for (int k = 0; k < nt; ++k) anyUV |= desc->UV && desc->tri_flags && (desc->tri_flags[k] & PG_TRI_HAS_UV);
    if (anyUV) uv.resize((size_t)nt * 6);
    ps.d.attrUV = anyUV ? 1 : 0;
    const float duv[6] = {0, 0, 1, 0, 1, 1};
    for (int k = 0; k < nt; ++k) {
        const int32_t *v = &desc->indices[3 * k];
        uint32_t flags = desc->tri_flags ? desc->tri_flags[k] : 0;
        int mat = desc->tri_material ? desc->tri_material[k] : 0;
        int light = desc->tri_light ? desc->tri_light[k] : -1;
        float4 *t = &tris[PG_TRI_STRIDE * (size_t)k];
        if (mat < 0 || mat >= desc->n_materials) PREP_FAIL(PG_ERR_INVALID, "triangle %d has out-of-range material %d", k, mat);
        if (light >= desc->n_lights) PREP_FAIL(PG_ERR_INVALID, "triangle %d has out-of-range light %d", k, light);
        if (flags & (PG_PRIM_INSTANCE | PG_PRIM_SPHERE)) {
            // TransformedPrimitive: the record carries the instance's index; Shape "sphere": the sphere's index, where a triangle has p0.x
            const bool inst = (flags & PG_PRIM_INSTANCE) != 0;
            if (!inst && (v[0] < 0 || v[0] >= desc->n_spheres || !desc->spheres)) PREP_FAIL(PG_ERR_INVALID, "primitive %d has out-of-range sphere index %d", k, v[0]);
            pgPrepIndexRecord(t, v[0], inst ? PG_PRIM_INSTANCE : PG_PRIM_SPHERE, mat, inst ? -1 : light);
            if (anyUV) memcpy(&uv[(size_t)k * 6], duv, sizeof(duv));
            continue;
        }
        for (int j = 0; j < 3; ++j)
            if (v[j] < 0 || v[j] >= desc->n_verts) PREP_FAIL(PG_ERR_INVALID, "triangle %d has out-of-range vertex index %d", k, v[j]);
        V3 p[3];
        for (int j = 0; j < 3; ++j) p[j] = mk(desc->P[3 * v[j]], desc->P[3 * v[j] + 1], desc->P[3 * v[j] + 2]);
        float tuv[6] = {0, 0, 1, 0, 1, 1};
        if (anyUV && (flags & PG_TRI_HAS_UV))
            for (int j = 0; j < 3; ++j) { tuv[2 * j] = desc->UV[2 * v[j]]; tuv[2 * j + 1] = desc->UV[2 * v[j] + 1]; }
        if (anyUV) memcpy(&uv[(size_t)k * 6], tuv, sizeof(tuv));
        V3 dpdu;
        if (!tri_dpdu(p[0], p[1], p[2], tuv, dpdu)) flags |= PG_TRI_BOGUS;  // triangle.cpp:309-317
        float fw, mw, lw;
        memcpy(&fw, &flags, 4); memcpy(&mw, &mat, 4); memcpy(&lw, &light, 4);
        t[0] = make_float4(p[0].x, p[0].y, p[0].z, fw);
        t[1] = make_float4(p[1].x, p[1].y, p[1].z, mw);
        t[2] = make_float4(p[2].x, p[2].y, p[2].z, lw);
    }
    if (desc->n_spheres > 0) ps.spheres.set(desc->spheres, sizeof(PgSphere) * (size_t)desc->n_spheres);
    ps.d.nSpheres = desc->n_spheres > 0 ? desc->n_spheres : 0;
    // per-vertex normals and (u, v), de-indexed like the positions, one 64-byte record per triangle (DScene::triAttr; only when some mesh has either);
    // tangents in an array of their own (only when some mesh has them)
    bool anyN = false, anyS = false;
    for (int k = 0; k < nt; ++k) {
        anyN |= desc->N && desc->tri_flags && (desc->tri_flags[k] & PG_TRI_HAS_N);
        anyS |= desc->S && desc->tri_flags && (desc->tri_flags[k] & PG_TRI_HAS_S);
    }
    ps.d.attrN = anyN ? 1 : 0;
    bool anyAlpha = false;  // k_trace's alpha masks read the (u, v) alone: from the compact array (24 B per triangle) they had before the attribute records
    if (anyN || anyUV) {
        std::vector<float> &a = ps.triAttr;
        a.assign((size_t)nt * 16, 0.f);
        for (int k = 0; k < nt; ++k) {
            float *r = &a[16 * (size_t)k];
            if (anyUV) memcpy(r + 10, &ps.uv[(size_t)k * 6], 6 * sizeof(float));
            if (!anyN || !(desc->tri_flags[k] & PG_TRI_HAS_N) || (desc->tri_flags[k] & (PG_PRIM_INSTANCE | PG_PRIM_SPHERE))) continue;
            const int32_t *v = &desc->indices[3 * k];
            for (int j = 0; j < 3; ++j) for (int c = 0; c < 3; ++c) r[3 * j + c] = desc->N[3 * v[j] + c];
        }
        for (int k = 0; k < nt && anyUV; ++k) anyAlpha |= (desc->tri_flags[k] & PG_TRI_ALPHA) != 0;
    }
    if (!anyAlpha) std::vector<float>().swap(ps.uv);
    if (anyS) {
        std::vector<float4> &a = ps.triS;
        a.assign((size_t)nt * 3, make_float4(0, 0, 0, 0));
        for (int k = 0; k < nt; ++k) {
            if (!(desc->tri_flags[k] & PG_TRI_HAS_S) || (desc->tri_flags[k] & (PG_PRIM_INSTANCE | PG_PRIM_SPHERE))) continue;
            const int32_t *v = &desc->indices[3 * k];
            for (int j = 0; j < 3; ++j) a[3 * (size_t)k + j] = make_float4(desc->S[3 * v[j]], desc->S[3 * v[j] + 1], desc->S[3 * v[j] + 2], 0.f);
        }
    }
    return PG_OK;
}
// --- texture graph: operands are earlier nodes (no cycles), nesting <= 3 levels (the unrolled evaluator of pg_texture.h)
inline int pgPrepTextures(const PgSceneDesc *desc, PreparedScene &ps, std::string &err) {
    std::vector<int> depth((size_t)(desc->n_textures > 0 ? desc->n_textures : 0), 1);
    auto refDepth = [&](const PgTexRef &r, int self) -> int { return r.tex < 0 ? 0 : ((r.tex >= self) ? 1000 : depth[r.tex]); };
    for (int i = 0; i < (int)depth.size(); ++i) {
        const PgTexture &t = desc->textures[i];
        if (t.type < PG_TEX_SCALE || t.type > PG_TEX_DOTS) PREP_FAIL(PG_ERR_UNSUPPORTED, "texture %d: unknown type %d", i, t.type);
        if (t.type >= PG_TEX_FBM && !desc->noise_perm) PREP_FAIL(PG_ERR_INVALID, "texture %d is a Perlin-noise texture, but the scene has no noise_perm table", i);
        if (t.type == PG_TEX_MARBLE && t.is_float) PREP_FAIL(PG_ERR_UNSUPPORTED, "texture %d: marble is a spectrum texture only (marble.cpp:39-42)", i);
        if (t.type == PG_TEX_IMAGEMAP && (t.image < 0 || t.image >= desc->n_images || desc->images[t.image].is_float != (t.is_float ? 1 : 0)))
            PREP_FAIL(PG_ERR_INVALID, "texture %d: image %d out of range or of the wrong texel type", i, t.image);
        int dmax = std::max(refDepth(t.tex1, i), std::max(refDepth(t.tex2, i), refDepth(t.amount, i)));
        if (dmax >= 1000) PREP_FAIL(PG_ERR_INVALID, "texture %d refers to a texture that is not defined before it", i);
        depth[i] = 1 + dmax;
        if (depth[i] > 3) PREP_FAIL(PG_ERR_UNSUPPORTED, "texture %d: operands nested %d deep (this build evaluates 3 levels)", i, depth[i]);
    }
    for (int i = 0; i < desc->n_textured; ++i) {
        const PgTexturedMaterial &tm = desc->textured[i];
        if (tm.kind < PG_KIND_MATTE || tm.kind > PG_KIND_MIX) PREP_FAIL(PG_ERR_UNSUPPORTED, "textured material %d: unknown kind %d", i, tm.kind);
        for (int k = 0; k < 5; ++k) if (tm.s[k].tex >= desc->n_textures) PREP_FAIL(PG_ERR_INVALID, "textured material %d: texture %d out of range", i, tm.s[k].tex);
        for (int k = 0; k < 4; ++k) if (tm.f[k].tex >= desc->n_textures) PREP_FAIL(PG_ERR_INVALID, "textured material %d: texture %d out of range", i, tm.f[k].tex);
        if (tm.kind != PG_KIND_MIX) continue;
        for (int j = 0; j < 2; ++j) {
            if (tm.sub[j] < 0 || tm.sub[j] >= desc->n_materials) PREP_FAIL(PG_ERR_INVALID, "textured material %d: mixed material %d out of range", i, tm.sub[j]);
            const PgMaterial &sm = desc->materials[tm.sub[j]];
            if (sm.type == PG_MAT_TEXTURED && sm.textured_index >= 0 && sm.textured_index < desc->n_textured && desc->textured[sm.textured_index].kind == PG_KIND_MIX) {
                const PgTexturedMaterial &t2 = desc->textured[sm.textured_index];
                for (int q = 0; q < 2; ++q)
                    if (t2.sub[q] >= 0 && t2.sub[q] < desc->n_materials && desc->materials[t2.sub[q]].type == PG_MAT_TEXTURED)
                        PREP_FAIL(PG_ERR_UNSUPPORTED, "textured material %d: textured mix materials nested more than two deep", i);
            }
        }
    }
    if (desc->n_images > 0) {
        if (!desc->images || !desc->texels || !desc->ewa_lut) PREP_FAIL(PG_ERR_INVALID, "images without texels / EWA weight table");
        for (int i = 0; i < desc->n_images; ++i) {
            const PgImage &im = desc->images[i];
            if (im.n_levels < 1 || im.n_levels > PG_MAX_MIP_LEVELS || im.width < 1 || im.height < 1 || (im.width & (im.width - 1)) || (im.height & (im.height - 1)))
                PREP_FAIL(PG_ERR_INVALID, "image %d: %d levels of %d x %d (MIPMap levels are powers of two)", i, im.n_levels, im.width, im.height);
            for (int l = 0; l < im.n_levels; ++l) {
                const int64_t sRes = std::max(1, im.width >> l), tRes = std::max(1, im.height >> l);
                if (im.level_offset[l] < 0 || im.level_offset[l] + sRes * tRes * (im.is_float ? 1 : 3) > desc->n_texel_floats)
                    PREP_FAIL(PG_ERR_INVALID, "image %d: level %d lies outside the texel array", i, l);
            }
        }
        ps.images.set(desc->images, sizeof(PgImage) * (size_t)desc->n_images);
        ps.texels.set(desc->texels, sizeof(float) * (size_t)desc->n_texel_floats);
        ps.ewaLut.set(desc->ewa_lut, sizeof(float) * 128);
    }
    if (desc->n_textures > 0 && desc->textures) ps.textures.set(desc->textures, sizeof(PgTexture) * (size_t)desc->n_textures);
    if (desc->n_textured > 0 && desc->textured) ps.textured.set(desc->textured, sizeof(PgTexturedMaterial) * (size_t)desc->n_textured);
    if (desc->n_bxdfs > 0 && desc->bxdfs) ps.bxdfs.set(desc->bxdfs, sizeof(PgBxDF) * (size_t)desc->n_bxdfs);
    return PG_OK;
}
// --- materials, lights, DScene::lightHot
inline int pgPrepMaterialsAndLights(const PgSceneDesc *desc, PreparedScene &ps, std::string &err) {
    const int nt = ps.nt;
    bool anyTextured = false;
    for (int i = 0; i < desc->n_materials; ++i) {
        const PgMaterial &m = desc->materials[i];
        if (m.type == PG_MAT_NONE) ps.hasNullMaterial = true;
        else if (m.type < PG_MAT_MATTE || m.type > PG_MAT_TEXTURED)
            PREP_FAIL(PG_ERR_UNSUPPORTED, "material %d: unknown type %d", i, m.type);
        if (m.type == PG_MAT_LOBES) ps.anyLobeMaterial = true;
        if (m.type == PG_MAT_TEXTURED) {
            anyTextured = true;
            if (m.textured_index < 0 || m.textured_index >= desc->n_textured || !desc->textured)
                PREP_FAIL(PG_ERR_INVALID, "material %d: textured_index %d out of range", i, m.textured_index);
        }
        if (m.n_bxdfs < 0 || m.n_bxdfs > PG_MAX_BXDFS || (m.n_bxdfs > 0 && (m.first_bxdf < 0 || m.first_bxdf + m.n_bxdfs > desc->n_bxdfs || !desc->bxdfs)))
            PREP_FAIL(PG_ERR_INVALID, "material %d: BxDF list [%d, +%d) is outside the scene's %d BxDFs", i, m.first_bxdf, m.n_bxdfs, desc->n_bxdfs);
        for (int j = 0; j < m.n_bxdfs; ++j) {
            const PgBxDF &bx = desc->bxdfs[m.first_bxdf + j];
            if (bx.type < PG_BXDF_LAMBERT_R || bx.type > PG_BXDF_FRESNEL_BLEND || bx.fresnel < PG_FRESNEL_NOOP || bx.fresnel > PG_FRESNEL_CONDUCTOR ||
                bx.n_scales < 0 || bx.n_scales > PG_MAX_BXDF_SCALES)
                PREP_FAIL(PG_ERR_UNSUPPORTED, "material %d: BxDF %d has unknown type %d / fresnel %d / %d scales", i, j, bx.type, bx.fresnel, bx.n_scales);
        }
    }
    ps.d.hasTextured = anyTextured ? 1 : 0;
    // device copy: a plastic's `roughness` becomes the TrowbridgeReitz alpha.  RoughnessToAlpha (microfacet.h:127-132) calls
    // logf; evaluating it here on the host uses the same libm as the reference build.
    ps.materials.assign(desc->materials, desc->materials + desc->n_materials);
    for (PgMaterial &m : ps.materials) {
        if (m.type != PG_MAT_PLASTIC) continue;
        float rough = m.roughness;
        if (m.remap_roughness) {
            rough = (rough < 1e-3f) ? 1e-3f : rough;  // std::max(roughness, (Float)1e-3)
            float x = logf(rough);
            rough = 1.62142f + 0.819955f * x + 0.1734f * x * x + 0.0171201f * x * x * x + 0.000640711f * x * x * x * x;
        }
        m.roughness = (0.001f < rough) ? rough : 0.001f;  // TrowbridgeReitzDistribution ctor: std::max(Float(0.001), alpha)
    }
    for (int i = 0; i < desc->n_lights; ++i)
        if (desc->lights[i].type == PG_LIGHT_INFINITE) {
            ps.d.hasInfinite = 1;
            const PgLight &l = desc->lights[i];
            const int64_t need = (int64_t)(2 * (int64_t)l.env_nu + 2) * l.env_nv + 2 * (int64_t)l.env_nv + 2;
            if (l.env_image < 0 || l.env_image >= desc->n_images || !desc->images || desc->images[l.env_image].is_float || l.env_nu < 1 || l.env_nv < 1 ||
                l.env_table < 0 || l.env_table + need > desc->n_env_floats || !desc->env_tables)
                PREP_FAIL(PG_ERR_INVALID, "light %d: infinite light without a valid radiance map / sampling distribution", i);
        }
    // projection / goniometric lights: sampled by the general shading kernels only
    for (int i = 0; i < desc->n_lights; ++i)
        if (desc->lights[i].type == PG_LIGHT_PROJECTION || desc->lights[i].type == PG_LIGHT_GONIO) {
            ps.anyImageLight = true;
            const PgLight &l = desc->lights[i];
            if (l.env_image >= desc->n_images || (l.env_image >= 0 && (!desc->images || desc->images[l.env_image].is_float)))
                PREP_FAIL(PG_ERR_INVALID, "light %d: map %d out of range or not an RGB image", i, l.env_image);
            if (l.type == PG_LIGHT_PROJECTION && !(l.screen[2] > l.screen[0] && l.screen[3] > l.screen[1])) PREP_FAIL(PG_ERR_INVALID, "light %d: empty projection screen bounds", i);
        }
    for (int i = 0; i < desc->n_lights; ++i)
        if (desc->lights[i].type < PG_LIGHT_AREA || desc->lights[i].type > PG_LIGHT_GONIO) PREP_FAIL(PG_ERR_UNSUPPORTED, "light %d: unknown type %d", i, desc->lights[i].type);
        else if (desc->lights[i].type == PG_LIGHT_AREA && (desc->lights[i].prim < 0 || desc->lights[i].prim >= nt))
            PREP_FAIL(PG_ERR_INVALID, "light %d has no emitting triangle", i);
    ps.lights.set(desc->lights, sizeof(PgLight) * (size_t)desc->n_lights);
    std::vector<float4> &hot = ps.lightHot;
    hot.assign((size_t)desc->n_lights * 5, make_float4(0, 0, 0, 0));
    for (int l = 0; l < desc->n_lights; ++l) {
        const PgLight &L = desc->lights[l];
        float ti, pi_, si;
        memcpy(&ti, &L.type, 4); memcpy(&pi_, &L.prim, 4); memcpy(&si, &L.two_sided, 4);
        hot[5 * (size_t)l] = make_float4(ti, pi_, si, L.area);
        hot[5 * (size_t)l + 1] = make_float4(L.L[0], L.L[1], L.L[2], 0.f);
        if (L.type == PG_LIGHT_AREA && L.prim >= 0 && L.prim < nt) for (int k = 0; k < 3; ++k) hot[5 * (size_t)l + 2 + k] = ps.tris[PG_TRI_STRIDE * (size_t)L.prim + k];
    }
    return PG_OK;
}
// --- sampler tables: the Halton permutations with their division constants, CMaxMinDist, the infinite lights' tables
inline int pgPrepSamplerTables(const PgSceneDesc *desc, PreparedScene &ps, std::string &err) {
    // (a scene rendered with the Sobol' sampler only may come without one: pg_render then refuses sampler = halton)
    const bool haltonTable = !(desc->n_perm_dims == 0 && desc->sobol_matrices);
    if (haltonTable && (desc->n_perm_dims < 5 || !desc->perms || !desc->perm_sums)) PREP_FAIL(PG_ERR_INVALID, "Halton permutation table missing (need >= 5 dims)");
    std::vector<int32_t> &primes = ps.primes;
    for (int c = 2; (int)primes.size() < desc->n_perm_dims; ++c) {
        bool is = true;
        for (int p : primes) { if (p * p > c) break; if (c % p == 0) { is = false; break; } }
        if (is) primes.push_back(c);
    }
    for (int i = 0; i < desc->n_perm_dims; ++i)
        if (desc->perm_sums[i + 1] - desc->perm_sums[i] != primes[i]) PREP_FAIL(PG_ERR_INVALID, "perm_sums[%d] does not match prime base %d", i, primes[i]);
    if (haltonTable) {
        ps.perms.set(desc->perms, sizeof(uint16_t) * (size_t)desc->perm_sums[desc->n_perm_dims]);
        ps.permSums.set(desc->perm_sums, sizeof(int32_t) * (size_t)(desc->n_perm_dims + 1));
        // per dimension, two int4: (base, offset of its digit permutation, m, L) with floor(a / base) = (t + ((a - t) >> 1)) >> (L - 1),
        // t = mulhi(m, a), for every 32-bit a (division by an invariant integer with a 33-bit multiplier: L = ceil(log2 base),
        // m = floor(2^32 (2^L - base) / base) + 1), and (invBase, invBase * perm[0] / (1 - invBase), 0, 0) as float bits: the two
        // per-dimension constants of ScrambledRadicalInverse (lowdiscrepancy.cpp:411, :422), evaluated here with the same float
        // operations in the same order as the kernels would (contraction off, IEEE division)
        std::vector<int32_t> &hd = ps.haltonDims;
        hd.assign(8 * primes.size(), 0);
        for (size_t i = 0; i < primes.size(); ++i) {
            const uint64_t b = (uint64_t)primes[i];
            int L = 0;
            while (((uint64_t)1 << L) < b) ++L;
            const uint64_t m = (((uint64_t)1 << 32) * (((uint64_t)1 << L) - b)) / b + 1;
            hd[8 * i] = primes[i]; hd[8 * i + 1] = desc->perm_sums[i]; hd[8 * i + 2] = (int32_t)(uint32_t)m; hd[8 * i + 3] = L;
            volatile float invBase = 1.f / (float)(uint32_t)primes[i];
            volatile float t1 = invBase * (float)desc->perms[desc->perm_sums[i]];
            volatile float t2 = 1 - invBase;
            volatile float tail = t1 / t2;
            const float ib = invBase, tl = tail;
            memcpy(&hd[8 * i + 4], &ib, 4); memcpy(&hd[8 * i + 5], &tl, 4);
        }
    }
    ps.d.nPermDims = desc->n_perm_dims;
    if (desc->cmaxmin) ps.cmaxmin.set(desc->cmaxmin, 17 * 32 * sizeof(uint32_t));  // the MaxMinDistSampler's generator matrices
    if (desc->n_env_floats > 0 && desc->env_tables) ps.envTables.set(desc->env_tables, sizeof(float) * (size_t)desc->n_env_floats);
    return PG_OK;
}
// --- alpha masks of triangle meshes
inline int pgPrepAlphaMasks(const PgSceneDesc *desc, PreparedScene &ps, std::string &err) {
    const int nt = ps.nt;
    bool anyAlpha = false;
    for (int k = 0; k < nt && desc->tri_flags; ++k)
        if ((desc->tri_flags[k] & PG_TRI_ALPHA) && !(desc->tri_flags[k] & (PG_PRIM_SPHERE | PG_PRIM_INSTANCE))) {
            anyAlpha = true;
            if (!desc->tri_alpha || !desc->alphas || desc->tri_alpha[k] < 0 || desc->tri_alpha[k] >= desc->n_alphas)
                PREP_FAIL(PG_ERR_INVALID, "triangle %d: PG_TRI_ALPHA without a valid alpha mask", k);
            const PgAlphaMask &am = desc->alphas[desc->tri_alpha[k]];
            if (am.alpha.tex >= desc->n_textures || am.shadow_alpha.tex >= desc->n_textures) PREP_FAIL(PG_ERR_INVALID, "triangle %d: alpha texture out of range", k);
        }
    ps.d.hasAlpha = anyAlpha ? 1 : 0;
    if (!anyAlpha) return PG_OK;
    ps.alphas.set(desc->alphas, sizeof(PgAlphaMask) * (size_t)desc->n_alphas);
    ps.triAlpha.set(desc->tri_alpha, sizeof(int) * (size_t)nt);
    // the masks in DAlphaTex form, if every one of them is a constant or a float image map under a (u, v) mapping
    std::vector<DAlphaTex> at((size_t)desc->n_alphas * 2);
    bool simple = getenv("PG_ALPHA_GENERAL") == nullptr;  // (tests: force the general evaluator)
    for (int k = 0; k < desc->n_alphas && simple; ++k)
        for (int which = 0; which < 2; ++which) {
            const PgAlphaMask &am = desc->alphas[k];
            const PgTexRef &r = which ? am.shadow_alpha : am.alpha;
            DAlphaTex &a = at[2 * (size_t)k + which];
            memset(&a, 0, sizeof(a));
            if (!(which ? am.has_shadow_alpha : am.has_alpha)) { a.image = -2; continue; }
            if (r.tex < 0) { a.image = -1; a.constant = r.v[0]; continue; }
            const PgTexture &tx = desc->textures[r.tex];
            if (tx.type != PG_TEX_IMAGEMAP || tx.mapping != PG_MAP_UV || tx.image < 0 || tx.image >= desc->n_images) { simple = false; break; }
            const PgImage &im = desc->images[tx.image];
            // (27 levels: beyond that MIPMap::Lookup's trilinear branch no longer lands on level 0 for a zero filter width)
            if (!im.is_float || im.n_levels < 1 || im.n_levels > 26 || im.width < 1 || im.height < 1) { simple = false; break; }
            a.su = tx.su; a.sv = tx.sv; a.du = tx.du; a.dv = tx.dv;
            a.width = im.width; a.height = im.height; a.wrap = im.wrap; a.image = tx.image; a.offset = im.level_offset[0];
        }
    if (simple) ps.alphaTex.swap(at);
    return PG_OK;
}
// --- subsurface scattering (the BSSRDFs, which material has one, the beam-diffusion tables), participating media
// (HomogeneousMedium) with the primitives' MediumInterfaces, and GridDensityMedium (the grids, which medium has one, the density values)
inline int pgPrepVolumes(const PgSceneDesc *desc, PreparedScene &ps, std::string &err) {
    const int nt = ps.nt;
    if (desc->n_bssrdfs > 0) {
        for (int k = 0; k < desc->n_bssrdfs; ++k) {
            const PgBSSRDF &b = desc->bssrdfs[k];
            const int64_t need = (int64_t)b.n_rho + b.n_radius + 2 * (int64_t)b.n_rho * b.n_radius + b.n_rho;
            if (b.n_rho < 2 || b.n_radius < 2 || b.table < 0 || b.table + need > desc->n_bssrdf_floats || b.match_material < 0 || b.match_material >= desc->n_materials ||
                b.a.tex >= desc->n_textures || b.b.tex >= desc->n_textures)
                PREP_FAIL(PG_ERR_INVALID, "BSSRDF %d: table / material / texture out of range", k);
        }
        for (int m = 0; m < desc->n_materials; ++m)
            if (desc->material_bssrdf[m] >= desc->n_bssrdfs) PREP_FAIL(PG_ERR_INVALID, "material %d: BSSRDF index out of range", m);
        ps.bssrdfs.set(desc->bssrdfs, sizeof(PgBSSRDF) * (size_t)desc->n_bssrdfs);
        ps.materialBssrdf.set(desc->material_bssrdf, sizeof(int32_t) * (size_t)desc->n_materials);
        ps.bssrdfTables.set(desc->bssrdf_tables, sizeof(float) * (size_t)desc->n_bssrdf_floats);
        ps.d.nBssrdfs = desc->n_bssrdfs;
    }
    const int nMedia = ps.nMedia = desc->n_media > 0 ? desc->n_media : 0;
    if (nMedia > 0 && !desc->media) PREP_FAIL(PG_ERR_INVALID, "n_media = %d without a media table", desc->n_media);
    if ((desc->tri_medium_inside != nullptr) != (desc->tri_medium_outside != nullptr)) PREP_FAIL(PG_ERR_INVALID, "tri_medium_inside and tri_medium_outside go together");
    if (desc->tri_medium_inside)
        for (int k = 0; k < nt; ++k)
            if (desc->tri_medium_inside[k] < -1 || desc->tri_medium_inside[k] >= nMedia || desc->tri_medium_outside[k] < -1 || desc->tri_medium_outside[k] >= nMedia)
                PREP_FAIL(PG_ERR_INVALID, "primitive %d: medium index out of range", k);
    if (nMedia > 0) ps.media.set(desc->media, sizeof(PgMedium) * (size_t)nMedia);
    if (desc->tri_medium_inside) { ps.triMediumIn.set(desc->tri_medium_inside, sizeof(int) * (size_t)nt); ps.triMediumOut.set(desc->tri_medium_outside, sizeof(int) * (size_t)nt); }
    if (desc->n_grids > 0) {
        int64_t nDensity = 0;
        for (int k = 0; k < desc->n_grids; ++k) {
            const PgDensityGrid &g = desc->grids[k];
            if (g.nx < 1 || g.ny < 1 || g.nz < 1 || g.density_offset < 0 || !(g.sigma_t > 0) || !(g.inv_max_density > 0))
                PREP_FAIL(PG_ERR_INVALID, "grid medium %d: malformed (%d x %d x %d, sigma_t %g)", k, g.nx, g.ny, g.nz, (double)g.sigma_t);
            nDensity = std::max<int64_t>(nDensity, g.density_offset + (int64_t)g.nx * g.ny * g.nz);
        }
        if (nDensity > desc->n_density_floats) PREP_FAIL(PG_ERR_INVALID, "grid media: %lld density values, %lld given", (long long)nDensity, (long long)desc->n_density_floats);
        for (int m = 0; m < nMedia; ++m) if (desc->media_grid[m] >= desc->n_grids) PREP_FAIL(PG_ERR_INVALID, "medium %d: grid index out of range", m);
        ps.grids.set(desc->grids, sizeof(PgDensityGrid) * (size_t)desc->n_grids);
        ps.mediaGrid.set(desc->media_grid, sizeof(int32_t) * (size_t)nMedia);
        ps.gridDensity.set(desc->grid_density, sizeof(float) * (size_t)nDensity);
        ps.d.nGrids = desc->n_grids;
    }
    return PG_OK;
}
// --- NoisePerm of the Perlin-noise textures, SobolSampler tables
inline int pgPrepNoiseAndSobol(const PgSceneDesc *desc, PreparedScene &ps, std::string &err) {
    if (desc->noise_perm) {
        for (int i = 0; i < 512; ++i) if (desc->noise_perm[i] < 0 || desc->noise_perm[i] > 255) PREP_FAIL(PG_ERR_INVALID, "noise_perm[%d] = %d is not a byte", i, desc->noise_perm[i]);
        ps.noisePerm.set(desc->noise_perm, sizeof(int) * 512);
    }
    if (desc->sobol_matrices) {
        if (!desc->vdc_sobol || !desc->vdc_sobol_inv) PREP_FAIL(PG_ERR_INVALID, "sobol_matrices without vdc_sobol / vdc_sobol_inv");
        ps.sobolMatrices.set(desc->sobol_matrices, sizeof(uint32_t) * 1024 * 52);
        ps.vdcSobol.set(desc->vdc_sobol, sizeof(uint64_t) * 25 * 52);
        ps.vdcSobolInv.set(desc->vdc_sobol_inv, sizeof(uint64_t) * 26 * 52);
    }
    return PG_OK;
}
// the longest BxDF list material mi can build, counted as the materials' ComputeScatteringFunctions add them (materials/*.cpp; MatEval, pg_material.h)
inline int pgPrepLobeCount(const PgSceneDesc *desc, int mi, int depth) {
    if (mi < 0 || mi >= desc->n_materials) return 0;
    const PgMaterial &m = desc->materials[mi];
    if (m.type != PG_MAT_TEXTURED) return std::min(std::max(m.n_bxdfs, 0), PG_MAX_BXDFS);
    const PgTexturedMaterial &tm = desc->textured[m.textured_index];
    switch (tm.kind) {
    case PG_KIND_MATTE: case PG_KIND_MIRROR: case PG_KIND_METAL: case PG_KIND_SUBSTRATE: return 1;
    case PG_KIND_PLASTIC: case PG_KIND_GLASS: return 2;
    case PG_KIND_UBER: return 5;
    case PG_KIND_TRANSLUCENT: return 4;
    case PG_KIND_MIX: return depth >= 3 ? PG_MAX_BXDFS : std::min(PG_MAX_BXDFS, pgPrepLobeCount(desc, tm.sub[0], depth + 1) + pgPrepLobeCount(desc, tm.sub[1], depth + 1));
    }
    return PG_MAX_BXDFS;
}
// --- shading plan: k_material's room per hit, the constant BxDF lists as PkLobe records, the shading classes, DScene::ext
inline void pgPrepShadingPlan(const PgSceneDesc *desc, PreparedScene &ps) {
    DScene &d = ps.d;
    const int nt = ps.nt;
    // k_material (materials evaluated ahead of the shading launch): room per hit = the longest BxDF list a material of this scene can
    // build.  Not for scenes with BSSRDF materials or grid media (their kernels evaluate inside), PG_MAT_PRE=0: nowhere.
    const char *mp = getenv("PG_MAT_PRE");
    if (d.hasTextured && desc->n_bssrdfs == 0 && d.nGrids == 0 && !d.hasNest && !(mp && atoi(mp) == 0)) {  // (hasNest: MODE 2 carries the second transform)
        // in RECORDS of 48 B (LobeBsdfT, pg_bxdf.h): one per BxDF, two where the hit's material is a mix (the ScaledBxDF factors)
        int stride = 1;
        for (int i = 0; i < desc->n_materials; ++i)
            if (desc->materials[i].type == PG_MAT_TEXTURED)
                stride = std::max(stride, pgPrepLobeCount(desc, i, 0) * (desc->textured[desc->materials[i].textured_index].kind == PG_KIND_MIX ? 2 : 1));
        ps.matStride = stride;
        // the constant lists once more as PkLobe records, for the kernel that reads k_material's (k_shade<3>)
        std::vector<float> &pk = ps.bxdfsPk;
        ps.matPk.assign((size_t)desc->n_materials, make_int2(0, 1));
        for (int i = 0; i < desc->n_materials; ++i) {
            const PgMaterial &m = desc->materials[i];
            if (m.type == PG_MAT_TEXTURED || m.n_bxdfs <= 0 || !desc->bxdfs) continue;
            bool scaled = false;
            for (int k = 0; k < m.n_bxdfs; ++k) scaled |= desc->bxdfs[m.first_bxdf + k].n_scales > 0;
            ps.matPk[i] = make_int2((int)(pk.size() / 12), scaled ? 2 : 1);
            for (int k = 0; k < m.n_bxdfs; ++k) {
                const PgBxDF &b = desc->bxdfs[m.first_bxdf + k];
                pk.resize(pk.size() + (scaled ? 24 : 12));
                float *q = pk.data() + pk.size() - (scaled ? 24 : 12);
                pg_pack_lobe(b, q);
                if (scaled) pg_pack_lobe_scales(b, q + 12);
            }
        }
        if (pk.empty()) pk.resize(12, 0.f);
    }
    // shading classes (k_shade_order): scenes whose materials evaluate textures / BxDF lists shade grouped by material.  Few
    // materials: each is a class (its textures stay with its waves as well); many: materials that run the same code
    // (type, kind, bump) share one.  PG_SHADE_ORDER=0: queue order, as scenes without such materials are shaded.
    const char *so = getenv("PG_SHADE_ORDER");
    ps.volOrder = ps.nMedia > 0 && d.nGrids == 0 && !(so && atoi(so) == 0);
    if (d.hasTextured && desc->n_materials > 1 && !(so && atoi(so) == 0)) {
        const int nClasses = PG_ORDER_CLASSES - 3;  // 0 .. 12; 13 = scattered in a medium (volpath), 14 = the ray escaped, 15 = no entry
        std::vector<unsigned char> matClass((size_t)desc->n_materials, 0);
        if (desc->n_materials <= nClasses) for (int i = 0; i < desc->n_materials; ++i) matClass[i] = (unsigned char)i;
        else {
            std::vector<int> sigs;
            for (int i = 0; i < desc->n_materials; ++i) {
                const PgMaterial &m = desc->materials[i];
                int sig = m.type;
                if (m.type == PG_MAT_TEXTURED) { const PgTexturedMaterial &tm = desc->textured[m.textured_index]; sig |= (tm.kind << 8) | (tm.has_bump ? 1 << 16 : 0); }
                size_t k = 0;
                while (k < sigs.size() && sigs[k] != sig) ++k;
                if (k == sigs.size()) sigs.push_back(sig);
                matClass[i] = (unsigned char)(k % (size_t)nClasses);
            }
        }
        ps.primClass.resize((size_t)nt);
        for (int k = 0; k < nt; ++k) ps.primClass[k] = matClass[desc->tri_material ? desc->tri_material[k] : 0];
    }
    // PG_FORCE_EXT=1 runs the general kernels on scenes that do not need them (tests: both paths agree bit for bit)
    const char *fe = getenv("PG_FORCE_EXT");
    d.ext = (d.hasTextured || d.nSpheres > 0 || d.nInstances > 0 || d.hasInfinite || ps.anyImageLight || ps.anyLobeMaterial || (fe && atoi(fe) != 0)) ? 1 : 0;
    d.nNodes = desc->n_nodes; d.nTris = nt; d.nLights = desc->n_lights; d.nMaterials = desc->n_materials;
    d.lightStrategy = desc->light_strategy;
}
// Light::Power() as the luminance PowerLightDistribution weighs a light by: diffuse.cpp:64-66, point.cpp:54, spot.cpp:74-76, distant.cpp:62-64
inline float pgPrepLightPowerY(const PgLight &l) {
    float P[3];
    for (int c = 0; c < 3; ++c) {
        float v = l.L[c];
        if (l.type == PG_LIGHT_POINT) v *= 4 * PG_PI;
        else if (l.type == PG_LIGHT_SPOT) { v *= 2; v *= PG_PI; v *= (1 - .5f * (l.cos_falloff_start + l.cos_total_width)); }
        else if (l.type == PG_LIGHT_DISTANT) { v *= PG_PI; v *= l.world_radius; v *= l.world_radius; }
        else if (l.type == PG_LIGHT_PROJECTION) { v = l.env_power[c] * v; v *= 2; v *= PG_PI; v *= (1.f - l.cos_total_width); }  // projection.cpp:93-99
        else if (l.type == PG_LIGHT_GONIO) v = (v * (4 * PG_PI)) * l.env_power[c];  // goniometric.cpp:54-58
        else if (l.type == PG_LIGHT_INFINITE) v = l.env_power[c] * (PG_PI * l.world_radius * l.world_radius);  // infinite.cpp:87-91
        else { v *= (float)(l.two_sided ? 2 : 1); v *= l.area; v *= PG_PI; }
        P[c] = v;
    }
    return 0.212671f * P[0] + 0.715160f * P[1] + 0.072169f * P[2];
}
// --- light sampling distributions (lightdistrib.cpp)
inline int pgPrepLightDistribution(const PgSceneDesc *desc, PreparedScene &ps, std::string &err) {
    DScene &d = ps.d;
    const int nl = desc->n_lights;
    if (nl <= 0) return PG_OK;
    const size_t stride = ps.distStride = 2 * (size_t)nl + 2;
    if (desc->light_strategy != PG_LIGHTS_SPATIAL) {
        // UniformLightDistribution (lightdistrib.cpp:68-71) / PowerLightDistribution (integrator.cpp:217-225, diffuse.cpp:64-66)
        std::vector<float> &tab = ps.distTable;
        tab.assign(stride, 0.f);
        float *func = tab.data(), *cdf = func + nl;
        for (int i = 0; i < nl; ++i) func[i] = desc->light_strategy == PG_LIGHTS_POWER ? pgPrepLightPowerY(desc->lights[i]) : 1;
        cdf[0] = 0;
        for (int i = 1; i < nl + 1; ++i) cdf[i] = cdf[i - 1] + func[i - 1] / nl;
        float funcInt = cdf[nl];
        if (funcInt == 0) { for (int i = 1; i < nl + 1; ++i) cdf[i] = (float)i / (float)nl; }
        else { for (int i = 1; i < nl + 1; ++i) cdf[i] /= funcInt; }
        tab[2 * nl + 1] = funcInt;
        return PG_OK;
    }
    // SpatialLightDistribution ctor, lightdistrib.cpp:96-125 (maxVoxels = 64)
    // a scene without geometry has no bound to divide into voxels and no surface to look a voxel up from: one voxel
    PgBVHNode root;
    memset(&root, 0, sizeof(root));
    if (desc->n_nodes > 0 && desc->nodes) root = desc->nodes[0];
    float diag[3];
    for (int i = 0; i < 3; ++i) { d.bmin[i] = root.bmin[i]; d.bmax[i] = root.bmax[i]; diag[i] = root.bmax[i] - root.bmin[i]; }
    int me = (diag[0] > diag[1] && diag[0] > diag[2]) ? 0 : ((diag[1] > diag[2]) ? 1 : 2);
    float bmax = diag[me];
    size_t total = 1;
    for (int i = 0; i < 3; ++i) {
        int nv = bmax > 0 ? (int)roundf(diag[i] / bmax * 64) : 1;
        d.nVoxels[i] = nv > 1 ? nv : 1;
        total *= (size_t)d.nVoxels[i];
    }
    // Dense table (every voxel up front: they are pure functions of the voxel) while it is small; beyond that the
    // voxels are computed on first touch like the reference's hash table (lightdistrib.cpp:135-230), into a pool.
    size_t denseLimit = (size_t)1 << 30;
    if (const char *e = getenv("PG_SPARSE_LIGHTS")) { if (atoi(e) != 0) denseLimit = 0; }
    if (total * stride * sizeof(float) <= denseLimit) { ps.denseVoxels = total; return PG_OK; }
    // (the exit vertices of subsurface paths look their light distribution up without the deferral the shading kernel has)
    if (d.nBssrdfs > 0) PREP_FAIL(PG_ERR_UNSUPPORTED, "subsurface scattering with a spatial light distribution beyond the dense table's size: use \"lightsamplestrategy\" \"power\" or \"uniform\"");
    if (d.nGrids > 0) PREP_FAIL(PG_ERR_UNSUPPORTED, "a grid medium with a spatial light distribution beyond the dense table's size: use \"lightsamplestrategy\" \"power\" or \"uniform\"");
    const size_t budget = (size_t)16 << 30;
    ps.nVoxelsTotal = (int)total;
    ps.poolSlots = (int)std::min<size_t>(total, std::max<size_t>(1, budget / (stride * sizeof(float))));
    d.sparseLights = 1;
    return PG_OK;
}

// The caller's description -> what pg_scene_create uploads.  PG_OK, or the status with its message in err; nothing here touches a device.
// traceDepth: TraceConfig::depth of the scene's launches (the LDS part of k_trace's stack).
inline int pg_prepare_scene(const PgSceneDesc *desc, int traceDepth, PreparedScene &out, std::string &err) {
    memset(&out.d, 0, sizeof(out.d));
    // primitives / nodes of object definitions follow the top-level ones (hosts that know no instancing leave the _all counts 0)
    out.nt = desc->n_prims_all > desc->n_tris ? desc->n_prims_all : desc->n_tris;
    out.nnAll = desc->n_nodes_all > desc->n_nodes ? desc->n_nodes_all : desc->n_nodes;
    PREP_STAGE(pgPrepBvh(desc, traceDepth, out, err));
    PREP_STAGE(pgPrepPrimitives(desc, out, err));
    PREP_STAGE(pgPrepTextures(desc, out, err));
    PREP_STAGE(pgPrepMaterialsAndLights(desc, out, err));
    PREP_STAGE(pgPrepSamplerTables(desc, out, err));
    PREP_STAGE(pgPrepAlphaMasks(desc, out, err));
    PREP_STAGE(pgPrepVolumes(desc, out, err));
    PREP_STAGE(pgPrepNoiseAndSobol(desc, out, err));
    pgPrepShadingPlan(desc, out);
    return pgPrepLightDistribution(desc, out, err);
}
#undef PREP_FAIL
#undef PREP_STAGE
#endif
