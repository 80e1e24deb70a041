// pg_triangle.h -- a triangle at shading time as device functions: its hot record (Tri, load_tri) and Triangle::Intersect's
// SurfaceInteraction from the hit's barycentrics (Isect, make_isect; hit_normal for the geometric normal alone), with SpawnRay.
//
// Used by every shading kernel of pg_kernels.hip and pg_direct.h, by the area lights of pg_light.h and by pg_hit.h, which adds
// the other shapes and the instance transforms.
#ifndef PG_TRIANGLE_H
#define PG_TRIANGLE_H
#include "pg_device.h"
#include "pg_kernels.h"

struct Tri { V3 p0, p1, p2; uint32_t flags; int material, light; };
PG_DEV Tri load_tri(const DScene &sc, int prim) {
    float4 a = sc.tris[PG_TRI_STRIDE * prim], b = sc.tris[PG_TRI_STRIDE * prim + 1], c = sc.tris[PG_TRI_STRIDE * prim + 2];
    Tri t;
    t.p0 = mk(a.x, a.y, a.z); t.p1 = mk(b.x, b.y, b.z); t.p2 = mk(c.x, c.y, c.z);
    t.flags = __float_as_uint(a.w); t.material = __float_as_int(b.w); t.light = __float_as_int(c.w);
    return t;
}
struct Isect { V3 p, pError, wo, n, ns, sdpdu, sdpdv, sdndu, sdndv; };  // n: geometric normal; ns, sd*: shading.n, shading.dpdu/dpdv/dndu/dndv (the last three feed bump mapping only)

PG_DEV V3 tri_normal(const Tri &t) {  // triangle.cpp:346-348
    V3 n = normalize(cross(t.p0 - t.p2, t.p1 - t.p2));
    if (t.flags & PG_TRI_FLIP_NORMAL) n = -n;
    return n;
}
PG_DEV void load_uv(const DScene &sc, int prim, uint32_t flags, float uv[6]) {  // triangle.h:98-108
    if (sc.attrUV && (flags & PG_TRI_HAS_UV)) tri_attr_uv(sc, prim, uv);
    else { uv[0] = 0; uv[1] = 0; uv[2] = 1; uv[3] = 0; uv[4] = 1; uv[5] = 1; }
}
// The tail of Triangle::Intersect (triangle.cpp:293-348) for the surviving hit.
// Per-vertex attribute a (N or S) of triangle prim interpolated with weights (w0, w1, w2): w0*a0 + w1*a1 + w2*a2.
PG_DEV V3 tri_interp(const float4 *attr, int prim, float w0, float w1, float w2) {
    const float4 a = attr[3 * (size_t)prim], b = attr[3 * (size_t)prim + 1], c = attr[3 * (size_t)prim + 2];
    return mk(a.x, a.y, a.z) * w0 + mk(b.x, b.y, b.z) * w1 + mk(c.x, c.y, c.z) * w2;
}
PG_DEV V3 tri_interp_normal(const DScene &sc, int prim, float w0, float w1, float w2) {  // the same with the per-vertex normals of DScene::triAttr
    float n[9];
    tri_attr_normals(sc, prim, n);
    return mk(n[0], n[1], n[2]) * w0 + mk(n[3], n[4], n[5]) * w1 + mk(n[6], n[7], n[8]) * w2;
}
// Triangle::Intersect's geometric normal for a hit with barycentrics (b0,b1,b2): Normalize(Cross(dp02, dp12)), flipped by
// reverseOrientation ^ transformSwapsHandedness (triangle.cpp:346-348), then made to face the interpolated shading normal
// when the mesh has per-vertex normals (SetShadingGeometry's Faceforward, interaction.cpp:79-81) -- full version below.
// The tail of Triangle::Intersect (triangle.cpp:293-419) for the surviving hit.
PG_DEV Isect make_isect(const DScene &sc, int prim, const Tri &t, float b0, float b1, float b2, V3 rayD) {
    Isect is;
    float uv[6];
    load_uv(sc, prim, t.flags, uv);
    V3 dpdu, dpdv;
    tri_dpdu_dpdv(t.p0, t.p1, t.p2, uv, dpdu, dpdv);
    float xAbsSum = (fabsf(b0 * t.p0.x) + fabsf(b1 * t.p1.x) + fabsf(b2 * t.p2.x));
    float yAbsSum = (fabsf(b0 * t.p0.y) + fabsf(b1 * t.p1.y) + fabsf(b2 * t.p2.y));
    float zAbsSum = (fabsf(b0 * t.p0.z) + fabsf(b1 * t.p1.z) + fabsf(b2 * t.p2.z));
    is.pError = mk(xAbsSum, yAbsSum, zAbsSum) * pgamma(7);
    is.p = t.p0 * b0 + t.p1 * b1 + t.p2 * b2;
    is.wo = normalize(-rayD);  // Interaction ctor, interaction.h:60
    is.n = tri_normal(t);
    is.ns = is.n;
    is.sdpdu = dpdu; is.sdpdv = dpdv;
    is.sdndu = is.sdndv = mk(0, 0, 0);
    const bool hasN = sc.attrN && (t.flags & PG_TRI_HAS_N), hasS = sc.triS && (t.flags & PG_TRI_HAS_S);
    if (hasN || hasS) {  // shading geometry, triangle.cpp:350-419 (dndu/dndv only feed ray differentials)
        V3 ns = is.n, ss = normalize(dpdu), ts;
        if (hasN) {
            V3 v = tri_interp_normal(sc, prim, b0, b1, b2);
            if (lensq(v) > 0) ns = normalize(v);
        }
        if (hasS) {
            V3 v = tri_interp(sc.triS, prim, b0, b1, b2);
            if (lensq(v) > 0) ss = normalize(v);
        }
        ts = cross(ss, ns);
        if (lensq(ts) > 0.f) { ts = normalize(ts); ss = cross(ts, ns); }
        else coordinate_system(ns, ss, ts);
        if (hasN) {  // dndu, dndv of the shading geometry, triangle.cpp:383-416
            const float d02x = uv[0] - uv[4], d02y = uv[1] - uv[5], d12x = uv[2] - uv[4], d12y = uv[3] - uv[5];
            float nv[9];
            tri_attr_normals(sc, prim, nv);
            const V3 n0 = mk(nv[0], nv[1], nv[2]), n1 = mk(nv[3], nv[4], nv[5]), n2 = mk(nv[6], nv[7], nv[8]);
            const V3 dn1 = n0 - n2, dn2 = n1 - n2;
            const float determinant = d02x * d12y - d02y * d12x;
            if ((double)fabsf(determinant) < 1e-8) {
                const V3 dn = cross(n2 - n0, n1 - n0);
                if (lensq(dn) != 0) coordinate_system(dn, is.sdndu, is.sdndv);
            } else {
                const float invDet = 1 / determinant;
                is.sdndu = (dn1 * d12y - dn2 * d02y) * invDet;
                is.sdndv = (dn1 * (-d12x) + dn2 * d02x) * invDet;
            }
        }
        if (t.flags & PG_TRI_REVERSE_ORIENTATION) ts = -ts;
        // SetShadingGeometry(ss, ts, ..., orientationIsAuthoritative = true), interaction.cpp:74-90
        is.ns = normalize(cross(ss, ts));
        if (dot(is.n, is.ns) < 0.f) is.n = -is.n;
        is.sdpdu = ss; is.sdpdv = ts;
    }
    return is;
}
// The geometric normal alone, as make_isect leaves it in isect.n (for Le() at a hit that is not shaded further).
PG_DEV V3 hit_normal(const DScene &sc, int prim, const Tri &t, float b0, float b1, float b2) {
    if ((sc.attrN && (t.flags & PG_TRI_HAS_N)) || (sc.triS && (t.flags & PG_TRI_HAS_S))) return make_isect(sc, prim, t, b0, b1, b2, mk(0, 0, 1)).n;
    return tri_normal(t);
}

PG_DEV void spawn_ray(const Isect &is, V3 d, V3 &o) { o = offset_ray_origin(is.p, is.pError, is.n, d); }  // interaction.h:64-67

#endif  // PG_TRIANGLE_H
