// pg_hit.h -- what every kernel that meets a closest hit shares, as device functions: the instance transforms above it (InstXf), the interaction of any shape
// in world space (hit_isect), an emitter's L there, the shadow ray and light pdf of EstimateDirect, what textures read of the hit
// (tex_hit_setup) and Material::Bump.
//
// Used by k_shade, k_material, k_through, k_sss_* (pg_kernels.hip), k_direct (pg_direct.h), k_scatter (pg_scatter.h) and the light queries' kernels
// (pg_lightquery.h).  Built from all the other pieces: included last.
#ifndef PG_HIT_H
#define PG_HIT_H
#include "pg_triangle.h"
#include "pg_sampler.h"
#include "pg_camera.h"
#include "pg_texture.h"
#include "pg_motion.h"
#include "pg_material.h"
#include "pg_light.h"

// ---- what every kernel that meets a closest hit shares: the hit's transforms, its SurfaceInteraction, an emitter's L there, and the two rays of
// EstimateDirect's light sample and BSDF sample.  One implementation each: the films are the reference's bit for bit, and two copies of a formula
// are two chances to round differently.

// One transform above a closest hit: InstanceToWorld, its inverse and IsIdentity of instance `inst` (< 0: none) -- the instance's own or, a moving one's,
// PrimitiveToWorld.Interpolate(r.time) as pg_motion.h left it in record off + i of `kept`.  Made once per hit: `outer` is the object instance's, `inner` the
// TransformedPrimitive's INSIDE the object of a hit two levels deep (DScene::hasNest).  It holds the two indices, not the addresses: those are formed where a
// matrix is read -- both sources are global memory --, so that no pointer is live across the interaction's arithmetic.  `kept` must exist whenever an instance
// is animated (moving() does not test it; k_sss_exit once fell back to the instance's own matrices under `animated && hitXf`): DScene::animXf and
// SssState::hitXf are both allocated exactly for a scene with motion (pg_abi.hip, `hasMotion`)
struct InstXf {
    const PgInstance *instances; const float *kept; int off;  // (uniform over a launch)
    int inst, i;
    PG_DEV bool some() const { return inst >= 0; }
    PG_DEV const float *moving() const { return instances[inst].animated ? kept + (size_t)PG_XF_STRIDE * ((size_t)off + i) : nullptr; }
    PG_DEV const float *i2w() const { const float *xf = moving(); return xf ? xf : instances[inst].i2w; }
    PG_DEV const float *w2i() const { const float *xf = moving(); return xf ? xf + 16 : instances[inst].w2i; }
    PG_DEV bool identity() const { const float *xf = moving(); return xf ? xf[32] != 0.f : instances[inst].identity != 0; }
};
// of the instance closest-hit result `i` was reached through: k_trace<.., XP_ANIM> computed a moving one's matrices for the accepted hit's ray and left them
// at animXf[i] -- the inner transform's in the buffer's second half
PG_DEV InstXf inst_xf(const DScene &sc, int inst, int i, bool inner = false) { return InstXf{sc.instances, sc.animXf, inner ? sc.nestXfOff : 0, inst, i}; }
// DScene::hasNest: a closest hit's instance word is outer + nInstances * (inner + 1); inner = -1 for a hit one level deep
PG_DEV void nest_decode(const DScene &sc, int &inst, int &inst2) { inst2 = -1; if (sc.hasNest && inst >= 0) { inst2 = inst / sc.nInstances - 1; inst = inst % sc.nInstances; } }
// The ray a hit under these transforms was computed on (primitive.cpp:80-82: the outer transform first): its direction, which every interaction's wo
// comes from ...
PG_DEV V3 shape_ray_dir(const InstXf &outer, const InstXf &inner, V3 rayD) {
    V3 d = rayD;
    if (outer.some()) d = m4_vec(outer.w2i(), rayD);
    if (inner.some()) d = m4_vec(inner.w2i(), d);
    return d;
}
// ... and the whole ray, which a quadric's interaction is computed from (instance_ray: the very operations of k_trace's, pg_sphere.h)
PG_DEV void shape_ray(const InstXf &outer, const InstXf &inner, float4 o4, V3 rayD, V3 &shapeRayO, V3 &shapeRayD) {
    shapeRayO = mk(o4.x, o4.y, o4.z);
    shapeRayD = rayD;
    if (outer.some()) { float dt; instance_ray(outer.w2i(), shapeRayO, rayD, shapeRayO, shapeRayD, dt); }
    if (inner.some()) { float dt; instance_ray(inner.w2i(), shapeRayO, shapeRayD, shapeRayO, shapeRayD, dt); }
}
// Sphere::Intersect's SurfaceInteraction (sphere.cpp:149-152): the shading geometry is the quadric's own
PG_DEV Isect sphere_isect(const SphereHit &sh) {
    Isect is;
    is.p = sh.p; is.pError = sh.pError; is.wo = sh.wo; is.n = sh.n; is.ns = sh.n; is.sdpdu = sh.dpdu;
    is.sdpdv = sh.dpdv; is.sdndu = sh.dndu; is.sdndv = sh.dndv;
    return is;
}
// InterpolatedPrimToWorld(*isect) of a hit reached through an object instance, transform.cpp:262-297
PG_DEV void isect_to_world(const float *i2w, const float *w2i, Isect &is) {
    Isect w;
    w.p = m4_point_err2(i2w, is.p, is.pError, w.pError);
    w.n = normalize(m4_normal(w2i, is.n));
    w.wo = normalize(m4_vec(i2w, is.wo));
    w.sdpdu = m4_vec(i2w, is.sdpdu);
    w.sdpdv = m4_vec(i2w, is.sdpdv);
    w.sdndu = m4_normal(w2i, is.sdndu); w.sdndv = m4_normal(w2i, is.sdndv);
    w.ns = normalize(m4_normal(w2i, is.ns));
    if (dot(w.ns, w.n) < 0.f) w.ns = -w.ns;  // Faceforward(shading.n, n)
    is = w;
}
// on the way out the inner transform first (TransformedPrimitive::Intersect returns through itself twice); an identity is skipped as the
// reference skips it (primitive.cpp:85: if (!InterpolatedPrimToWorld.IsIdentity()))
PG_DEV void isect_to_world(const InstXf &outer, const InstXf &inner, Isect &is) {
    if (inner.some() && !inner.identity()) isect_to_world(inner.i2w(), inner.w2i(), is);
    if (outer.some() && !outer.identity()) isect_to_world(outer.i2w(), outer.w2i(), is);
}
// A quadric hit's (u, v) and geometric dpdu / dpdv, in the shape's space: what textures read besides the interaction (tex_hit_setup)
struct QuadricUv { bool on; float u, v; V3 dpdu, dpdv; };  // (on: the hit is on a quadric at all)
// The SurfaceInteraction of closest hit h4 on primitive `prim`, found by ray (o4, rayD) under these transforms: the three stages above in one
PG_DEV Isect hit_isect(const DScene &sc, const InstXf &outer, const InstXf &inner, float4 o4, V3 rayD, float4 h4, int prim, const Tri &tri, QuadricUv &quv) {
    Isect is;
    quv.on = (tri.flags & PG_PRIM_SPHERE) != 0;
    quv.u = quv.v = 0; quv.dpdu = quv.dpdv = mk(0, 0, 0);
    if (quv.on) {  // the hit record of a sphere carries tHit: Sphere::Intersect's interaction from the ray and the root
        V3 shapeRayO, shapeRayD;
        shape_ray(outer, inner, o4, rayD, shapeRayO, shapeRayD);
        const SphereHit sh = sphere_interaction(sc.spheres[__float_as_int(tri.p0.x)], shapeRayO, shapeRayD, h4.y);
        is = sphere_isect(sh);
        quv.u = sh.u; quv.v = sh.v; quv.dpdu = sh.dpdu; quv.dpdv = sh.dpdv;
    } else is = make_isect(sc, prim, tri, h4.y, h4.z, h4.w, shape_ray_dir(outer, inner, rayD));
    isect_to_world(outer, inner, is);
    return is;
}
// DiffuseAreaLight::L(intr, w) (diffuse.h:56-58) with the emitter's geometric normal n
PG_DEV Spec area_light_l(const PgLight &l, V3 n, V3 w) { return (l.two_sided || dot(n, w) > 0) ? sp3(l.L[0], l.L[1], l.L[2]) : sp(0); }
// ... at closest hit h4 of ray (o4, rayD) on the emitter's primitive, back along the ray (integrator.cpp:204 lightIsect.Le(-wi)): the kernels that meet
// the hit without building its interaction.  An emitter lies under no instance (api.cpp:1408-1409: an object definition's shapes take no area light), so the ray is the
// shape's.  SPHERES: the scene may have quadrics at all (DScene::ext)
template <bool SPHERES>
PG_DEV Spec area_light_le(const DScene &sc, const PgLight &l, int prim, const Tri &tri, float4 h4, float4 o4, V3 rayD) {
    V3 nrm;
    if (SPHERES && (tri.flags & PG_PRIM_SPHERE)) nrm = sphere_interaction(sc.spheres[__float_as_int(tri.p0.x)], mk(o4.x, o4.y, o4.z), rayD, h4.y).n;
    else nrm = hit_normal(sc, prim, tri, h4.y, h4.z, h4.w);
    return area_light_l(l, nrm, -rayD);
}
// VisibilityTester's ray from (p, pError, n) to the light sample: p0.SpawnRayTo(p1), interaction.h:73-78 -- as a shadow-queue record (tag: what the
// queue's consumer finds the vertex by); returns the ray's direction
PG_DEV V3 shadow_ray_to(V3 p, V3 pError, V3 n, const LightSample &ls, int tag, float4 &o4, float4 &d4) {
    const V3 origin = offset_ray_origin(p, pError, n, ls.p - p);
    const V3 target = offset_ray_origin(ls.p, ls.pError, ls.n, origin - ls.p);
    const V3 d = target - origin;
    o4 = make_float4(origin.x, origin.y, origin.z, 1 - PG_SHADOW_EPS);
    d4 = make_float4(d.x, d.y, d.z, __int_as_float(tag));
    return d;
}
// light.Pdf_Li(ref, wi) of EstimateDirect's BSDF-sampled direction (integrator.cpp:175-178), for the ray (ro, wi) spawned at refP: an infinite light's
// from its distribution (lightPrim = -1 - its number: no geometry to test); an area light's Shape::Pdf, which intersects the light's own shape
// (shape.cpp:72-87, diffuse.cpp:83-87) -- one triangle test counted in nLightTests, whose hit on a degenerate triangle (PG_TRI_BOGUS) the reference's
// Triangle::Intersect refuses --, or Sphere::Pdf (sphere.cpp:292-305): the cone's for a reference point outside (`inside`: sphere_ref_inside, or a partial sphere)
template <bool EXT>
PG_DEV float mis_light_pdf(const DScene &sc, int lightPrim, float lightArea, bool inside, V3 refP, V3 ro, V3 wi, unsigned int &nLightTests) {
    float lightPdf = 0;
    if (EXT && lightPrim < 0) lightPdf = env_pdf_li(sc, sc.lights[-1 - lightPrim], wi);
    const Tri lt = load_tri(sc, lightPrim < 0 ? 0 : lightPrim);
    float t, lb0, lb1, lb2;
    if (EXT && lightPrim >= 0 && (lt.flags & PG_PRIM_SPHERE)) {
        const PgSphere &ls = sc.spheres[__float_as_int(lt.p0.x)];
        if (!inside) lightPdf = sphere_cone_pdf(ls, refP);
        else if (sphere_test(ls, ro, wi, PG_INF, t)) {  // Shape::Pdf, shape.cpp:72-87
            const SphereHit sh = sphere_interaction(ls, ro, wi, t);
            float pdf = lensq(refP - sh.p) / (absdot(sh.n, -wi) * lightArea);
            if (isinf(pdf)) pdf = 0.f;
            lightPdf = pdf;
        }
    } else {
        if (lightPrim >= 0) ++nLightTests;
        if (lightPrim >= 0 && tri_test(lt.p0, lt.p1, lt.p2, ro, wi, PG_INF, t, lb0, lb1, lb2) && !(lt.flags & PG_TRI_BOGUS)) {
            const V3 lp = lt.p0 * lb0 + lt.p1 * lb1 + lt.p2 * lb2;
            const V3 ln = normalize(cross(lt.p0 - lt.p2, lt.p1 - lt.p2));
            float pdf = lensq(refP - lp) / (absdot(ln, -wi) * lightArea);
            if (isinf(pdf)) pdf = 0.f;
            lightPdf = pdf;
        }
    }
    return lightPdf;
}
// what mis_light_pdf needs of the sampled light: (lightPrim, inside) for the reference point (p, pError, n)
PG_DEV void mis_light_of(const DScene &sc, const LightHot &lh, int lightNum, V3 p, V3 pError, V3 n, int &lightPrim, bool &inside) {
    lightPrim = lh.type == PG_LIGHT_INFINITE ? -1 - lightNum : lh.prim;
    inside = false;
    if (lh.type == PG_LIGHT_AREA && (lh.tri.flags & PG_PRIM_SPHERE)) {
        const PgSphere &lsph = sc.spheres[__float_as_int(lh.tri.p0.x)];
        inside = lsph.shape != PG_SHAPE_SPHERE || sphere_ref_inside(lsph, p, pError, n);
    }
}
// What textures read of the SurfaceInteraction at main-queue entry i: (u, v), p and ComputeDifferentials' outputs
// (interaction.cpp:101-147).  quv: a quadric hit's (u, v) and geometric dpdu / dpdv; filmX / filmY: the camera sample's pFilm
PG_DEV void tex_hit_setup(const DScene &sc, const PgRenderDesc &rd, const RayQueue &qin, int i, int slot, int prim, const Tri &tri, float4 h4, V3 rayD, const InstXf &outer,
                          const InstXf &inner, const QuadricUv &quv, const Isect &is, int4 meta, float filmX, float filmY,
                          bool tileSerial, bool pixelArrays, uint64_t index, TexHit &th, const float4 *stL) {
    th.p = is.p;
    V3 gdpdu, gdpdv;  // the geometric dpdu / dpdv (not the shading ones)
    if (quv.on) { th.u = quv.u; th.v = quv.v; gdpdu = quv.dpdu; gdpdv = quv.dpdv; }
    else {
        float uv[6];
        load_uv(sc, prim, tri.flags, uv);
        tri_dpdu_dpdv(tri.p0, tri.p1, tri.p2, uv, gdpdu, gdpdv);
        th.u = h4.y * uv[0] + h4.z * uv[2] + h4.w * uv[4];  // uvHit, triangle.cpp:332
        th.v = h4.y * uv[1] + h4.z * uv[3] + h4.w * uv[5];
    }
    if (inner.some() && !inner.identity()) { gdpdu = m4_vec(inner.i2w(), gdpdu); gdpdv = m4_vec(inner.i2w(), gdpdv); }  // (the inner transform first)
    if (outer.some() && !outer.identity()) { gdpdu = m4_vec(outer.i2w(), gdpdu); gdpdv = m4_vec(outer.i2w(), gdpdv); }
    th.dpdx = th.dpdy = mk(0, 0, 0);
    th.dudx = th.dvdx = th.dudy = th.dvdy = 0;
    if (meta.w & PG_META_HASDIFF) {  // SurfaceInteraction::ComputeDifferentials, interaction.cpp:101-147
        const float4 o4 = qin.o[i];
        const V3 rayO = mk(o4.x, o4.y, o4.z);
        V3 rxO, rxD, ryO, ryD;
        if (rd.camera_type == 3) {  // the realistic camera: k_generate traced the shifted rays through the lens and kept the scaled differentials by slot
            const float4 *df = lens_frame(stL)->differentials + 3 * (size_t)slot;
            const float4 a = df[0], b = df[1], c = df[2];
            rxO = mk(a.x, a.y, a.z); rxD = mk(a.w, b.x, b.y); ryO = mk(b.z, b.w, c.x); ryD = mk(c.y, c.z, c.w);
        } else {
        float l0 = 0, l1 = 0;
        if (tileSerial) { l0 = sc.ts[slot].lens0; l1 = sc.ts[slot].lens1; }  // the camera sample's pLens, kept by k_ts_generate
        else if (pixelArrays) { int d2 = 1 << 6; tsb_get2d(sc, meta.x, meta.y, d2, l0, l1); }  // (its second 2D dimension)
        else if (rd.lens_radius > 0) { l0 = halton_sample(sc, rd, index, 3); l1 = halton_sample(sc, rd, index, 4); }
        // the camera sample's time again (its third number), for the camera-to-world transform of that moment
        float uTime = 0;
        if (rd.camera_animated) {
            if (tileSerial) uTime = sc.ts[slot].time;
            else if (pixelArrays) { int d1 = 0; uTime = tsb_get1d(sc, meta.x, meta.y, d1); }
            else uTime = halton_sample(sc, rd, index, 2);
        }
        if (rd.camera_animated) {  // (two calls: one pointer that is either the description's matrix or a private array would be a generic one)
            float c2w[16];
            camera_matrix_at(rd, camera_time(rd, uTime), c2w);
            camera_differentials(rd, c2w, filmX, filmY, l0, l1, rayO, rayD, rxO, rxD, ryO, ryD);
        } else camera_differentials(rd, rd.camera_to_world, filmX, filmY, l0, l1, rayO, rayD, rxO, rxD, ryO, ryD);
        }
        const V3 n = is.n, p = is.p;
        const float dd = dot(n, p);
        const float tx = -(dot(n, rxO) - dd) / dot(n, rxD);
        const float ty = -(dot(n, ryO) - dd) / dot(n, ryD);
        if (!(isinf(tx) || isnan(tx)) && !(isinf(ty) || isnan(ty))) {
            const V3 px = rxO + rxD * tx, py = ryO + ryD * ty;
            th.dpdx = px - p;
            th.dpdy = py - p;
            int d0, d1;
            if (fabsf(n.x) > fabsf(n.y) && fabsf(n.x) > fabsf(n.z)) { d0 = 1; d1 = 2; }
            else if (fabsf(n.y) > fabsf(n.z)) { d0 = 0; d1 = 2; }
            else { d0 = 0; d1 = 1; }
            auto comp = [](V3 v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); };
            const float A00 = comp(gdpdu, d0), A01 = comp(gdpdv, d0), A10 = comp(gdpdu, d1), A11 = comp(gdpdv, d1);
            const float Bx0 = comp(px, d0) - comp(p, d0), Bx1 = comp(px, d1) - comp(p, d1);
            const float By0 = comp(py, d0) - comp(p, d0), By1 = comp(py, d1) - comp(p, d1);
            const float det = A00 * A11 - A01 * A10;  // SolveLinearSystem2x2, transform.cpp:41-49
            if (!(fabsf(det) < 1e-10f)) {
                th.dudx = (A11 * Bx0 - A01 * Bx1) / det; th.dvdx = (A00 * Bx1 - A10 * Bx0) / det;
                if (isnan(th.dudx) || isnan(th.dvdx)) th.dudx = th.dvdx = 0;
                th.dudy = (A11 * By0 - A01 * By1) / det; th.dvdy = (A00 * By1 - A10 * By0) / det;
                if (isnan(th.dudy) || isnan(th.dvdy)) th.dudy = th.dvdy = 0;
            }
        }
    }
}
// (the same from the hit's instance words and a quadric's values apart, for k_shade, which holds no InstXf across its vertex)
PG_DEV void tex_hit_setup(const DScene &sc, const PgRenderDesc &rd, const RayQueue &qin, int i, int slot, int prim, const Tri &tri, float4 h4, V3 rayD, int inst, int inst2,
                          bool onSphere, float sphU, float sphV, V3 sphDpdu, V3 sphDpdv, const Isect &is, int4 meta, float filmX, float filmY,
                          bool tileSerial, bool pixelArrays, uint64_t index, TexHit &th, const float4 *stL) {
    const QuadricUv quv = {onSphere, sphU, sphV, sphDpdu, sphDpdv};
    tex_hit_setup(sc, rd, qin, i, slot, prim, tri, h4, rayD, inst_xf(sc, inst, i), inst_xf(sc, inst2, i, true), quv, is, meta, filmX, filmY, tileSerial, pixelArrays, index, th, stL);
}
// Material::Bump (material.cpp:46-85) of the material whose BSDF this is: its own bump map, or -- through mix materials, whose
// BSDF is their first material's -- the first material's
template <int W = 0>
PG_DEV void material_bump(const DScene &sc, int material, const TexHit &th, Isect &is) {
    int bm = material;
    for (int lvl = 0; lvl < 4; ++lvl) {
        const PgMaterial &mm = sc.materials[bm];
        if (mm.type != PG_MAT_TEXTURED) break;
        const PgTexturedMaterial &tmm = sc.textured[mm.textured_index];
        if (tmm.kind == PG_KIND_MIX) { if (tmm.sub[0] < 0) break; bm = tmm.sub[0]; continue; }
        if (tmm.has_bump) {
            TexHit ev = th;
            float du = .5f * (fabsf(th.dudx) + fabsf(th.dudy));
            if (du == 0) du = .0005f;
            ev.p = th.p + is.sdpdu * du; ev.u = th.u + du; ev.v = th.v + 0.f;
            const float uDisplace = TexEval<PG_TEX_DEPTH, W>::f(*sc.self, tmm.bump, ev);
            float dv = .5f * (fabsf(th.dvdx) + fabsf(th.dvdy));
            if (dv == 0) dv = .0005f;
            ev.p = th.p + is.sdpdv * dv; ev.u = th.u + 0.f; ev.v = th.v + dv;
            const float vDisplace = TexEval<PG_TEX_DEPTH, W>::f(*sc.self, tmm.bump, ev);
            const float displace = TexEval<PG_TEX_DEPTH, W>::f(*sc.self, tmm.bump, th);
            const V3 bdpdu = (is.sdpdu + is.ns * ((uDisplace - displace) / du)) + is.sdndu * displace;
            const V3 bdpdv = (is.sdpdv + is.ns * ((vDisplace - displace) / dv)) + is.sdndv * displace;
            is.ns = normalize(cross(bdpdu, bdpdv));  // SetShadingGeometry(..., false), interaction.cpp:72-89
            if (dot(is.ns, is.n) < 0.f) is.ns = -is.ns;
            is.sdpdu = bdpdu; is.sdpdv = bdpdv;
        }
        break;
    }
}

#endif  // PG_HIT_H
