// pg_light.h -- Light::Sample_Li / Pdf_Li / Le as device functions: spot, projection, goniometric, distant, point, diffuse area
// (triangles and quadrics) and infinite area lights, the hot record of the light a lane sampled (LightHot), and the light
// distributions (light_distribution; sample_discrete stays in pg_kernels.hip).
//
// Used by k_shade, k_sss_exit, k_resolve*, k_light_tables* (pg_kernels.hip), k_direct (pg_direct.h), mis_light_pdf (pg_hit.h) and the light queries'
// k_light_sample / k_emitted (pg_lightquery.h).
#ifndef PG_LIGHT_H
#define PG_LIGHT_H
#include "pg_device.h"
#include "pg_sphere.h"
#include "pg_kernels.h"
#include "pg_texture.h"
#include "pg_triangle.h"

struct LightSample { V3 p, n, pError; };
// SpotLight::Falloff, spot.cpp:62-72
PG_DEV float spot_falloff(const PgLight &l, V3 w) {
    V3 wl = normalize(mk(l.w2l[0] * w.x + l.w2l[1] * w.y + l.w2l[2] * w.z, l.w2l[3] * w.x + l.w2l[4] * w.y + l.w2l[5] * w.z,
                         l.w2l[6] * w.x + l.w2l[7] * w.y + l.w2l[8] * w.z));  // Transform::operator()(Vector3), transform.h:233-239
    float cosTheta = wl.z;
    if (cosTheta < l.cos_total_width) return 0;
    if (cosTheta >= l.cos_falloff_start) return 1;
    float delta = (cosTheta - l.cos_total_width) / (l.cos_falloff_start - l.cos_total_width);
    return (delta * delta) * (delta * delta);
}
// ---- Sphere as the shape of a DiffuseAreaLight: Sphere::Sample / ::Pdf, shapes/sphere.cpp:205-305
PG_DEV bool sphere_ref_inside(const PgSphere &s, V3 refp, V3 refErr, V3 refn) {  // sphere.cpp:223-226, :294-297
    const V3 pCenter = m4_point(s.o2w, mk(0, 0, 0));
    const V3 pOrigin = offset_ray_origin(refp, refErr, refn, pCenter - refp);
    return lensq(pOrigin - pCenter) <= s.radius * s.radius;
}
PG_DEV float sphere_cone_pdf(const PgSphere &s, V3 refp) {  // sphere.cpp:301-304, UniformConePdf sampling.cpp:132-134
    const V3 pCenter = m4_point(s.o2w, mk(0, 0, 0));
    const float sinThetaMax2 = s.radius * s.radius / lensq(refp - pCenter);
    const float cosThetaMax = sqrtf(pmax(0.f, 1 - sinThetaMax2));
    return 1 / (2 * PG_PI * (1 - cosThetaMax));
}
PG_DEV LightSample sphere_sample(const PgSphere &s, V3 refp, V3 refErr, V3 refn, float u0, float u1, float &pdf) {
    LightSample it;
    const float radius = s.radius;
    const V3 pCenter = m4_point(s.o2w, mk(0, 0, 0));
    if (sphere_ref_inside(s, refp, refErr, refn)) {  // uniform over the area (sphere.cpp:205-217), then to solid angle (:227-239)
        const float z = 1 - 2 * u0;  // UniformSampleSphere, sampling.cpp:98-103
        const float r = sqrtf(pmax(0.f, 1.f - z * z));
        const float phi = 2 * PG_PI * u1;
        float sP, cP;
        pg_sincosf(phi, &sP, &cP);
        V3 pObj = mk(r * (float)cP, r * (float)sP, z) * radius;
        it.n = normalize(m4_normal(s.w2o, pObj));
        if (s.reverse_orientation) it.n = it.n * -1.f;
        pObj = pObj * (radius / sqrtf(lensq(pObj)));
        it.p = m4_point_err2(s.o2w, pObj, vabs(pObj) * pgamma(5), it.pError);
        pdf = 1 / (s.phi_max * radius * (s.z_max - s.z_min));
        V3 wi = it.p - refp;
        if (lensq(wi) == 0) pdf = 0;
        else {
            wi = normalize(wi);
            pdf *= lensq(refp - it.p) / absdot(it.n, -wi);
        }
        if (isinf(pdf)) pdf = 0.f;
        return it;
    }
    // uniformly inside the subtended cone, sphere.cpp:241-289
    const float dc = sqrtf(lensq(refp - pCenter));
    const float invDc = 1 / dc;
    const V3 wc = (pCenter - refp) * invDc;
    V3 wcX, wcY;
    coordinate_system(wc, wcX, wcY);
    const float sinThetaMax = radius * invDc;
    const float sinThetaMax2 = sinThetaMax * sinThetaMax;
    const float invSinThetaMax = 1 / sinThetaMax;
    const float cosThetaMax = sqrtf(pmax(0.f, 1 - sinThetaMax2));
    float cosTheta = (cosThetaMax - 1) * u0 + 1;
    float sinTheta2 = 1 - cosTheta * cosTheta;
    if (sinThetaMax2 < 0.00068523f) {  // sin^2(1.5 deg): the reference's small-angle series
        sinTheta2 = sinThetaMax2 * u0;
        cosTheta = sqrtf(1 - sinTheta2);
    }
    const float cosAlpha = sinTheta2 * invSinThetaMax + cosTheta * sqrtf(pmax(0.f, 1.f - sinTheta2 * invSinThetaMax * invSinThetaMax));
    const float sinAlpha = sqrtf(pmax(0.f, 1.f - cosAlpha * cosAlpha));
    const float phi = u1 * 2 * PG_PI;
    float sP, cP;
    pg_sincosf(phi, &sP, &cP);
    // SphericalDirection(sinAlpha, cosAlpha, phi, -wcX, -wcY, -wc), geometry.h:1461-1466
    const V3 nWorld = (-wcX) * (sinAlpha * (float)cP) + (-wcY) * (sinAlpha * (float)sP) + (-wc) * cosAlpha;
    const V3 pWorld = pCenter + nWorld * radius;
    it.p = pWorld;
    it.pError = vabs(pWorld) * pgamma(5);
    it.n = nWorld;
    if (s.reverse_orientation) it.n = it.n * -1.f;
    pdf = 1 / (2 * PG_PI * (1 - cosThetaMax));
    return it;
}

// Cylinder::Sample(u, pdf), cylinder.cpp:208-223; Disk::Sample(u, pdf), disk.cpp:128-137
PG_DEV LightSample quadric_sample_area(const PgSphere &s, float u0, float u1, float &pdf) {
    LightSample it;
    if (s.shape == PG_SHAPE_CYLINDER) {
        const float z = plerp(u0, s.z_min, s.z_max);
        const float phi = u1 * s.phi_max;
        float sP, cP;
        pg_sincosf(phi, &sP, &cP);
        V3 pObj = mk(s.radius * (float)cP, s.radius * (float)sP, z);
        it.n = normalize(m4_normal(s.w2o, mk(pObj.x, pObj.y, 0)));
        if (s.reverse_orientation) it.n = it.n * -1.f;
        const float hitRad = sqrtf(pObj.x * pObj.x + pObj.y * pObj.y);
        pObj.x *= s.radius / hitRad;
        pObj.y *= s.radius / hitRad;
        it.p = m4_point_err2(s.o2w, pObj, vabs(mk(pObj.x, pObj.y, 0)) * pgamma(3), it.pError);
    } else {
        float px, py;
        concentric_sample_disk(u0, u1, px, py);
        const V3 pObj = mk(px * s.radius, py * s.radius, s.height);
        it.n = normalize(m4_normal(s.w2o, mk(0, 0, 1)));
        if (s.reverse_orientation) it.n = it.n * -1.f;
        it.p = m4_point_err2(s.o2w, pObj, mk(0, 0, 0), it.pError);
    }
    pdf = 1 / s.area;
    return it;
}

// Triangle::Sample(u, pdf), triangle.cpp:582-607 with UniformSampleTriangle, sampling.cpp:154-157
PG_DEV LightSample tri_sample_area(const DScene &sc, const Tri &t, int prim, float area, float u0, float u1, float &pdf) {
    LightSample ls;
    float su0 = sqrtf(u0);
    float b0 = 1 - su0, b1 = u1 * su0;
    float b2 = (1 - b0 - b1);
    ls.p = t.p0 * b0 + t.p1 * b1 + t.p2 * b2;
    ls.n = normalize(cross(t.p1 - t.p0, t.p2 - t.p0));
    if (sc.attrN && (t.flags & PG_TRI_HAS_N)) {  // triangle.cpp:593-597: orientation follows the shading normal
        V3 ns = tri_interp_normal(sc, prim, b0, b1, b2);
        if (dot(ls.n, ns) < 0.f) ls.n = -ls.n;
    } else if (t.flags & PG_TRI_FLIP_NORMAL) ls.n = ls.n * -1.f;
    V3 pAbsSum = vabs(t.p0 * b0) + vabs(t.p1 * b1) + vabs(t.p2 * b2);
    ls.pError = pAbsSum * pgamma(6);
    pdf = 1 / area;
    return ls;
}
// Shape::Sample(ref, u, pdf), shape.cpp:56-70: the area sample's pdf with respect to solid angle at refp
PG_DEV void area_to_solid_angle(V3 refp, const LightSample &ls, float &pdf) {
    V3 w = ls.p - refp;
    if (lensq(w) == 0) pdf = 0;
    else {
        w = normalize(w);
        pdf *= lensq(refp - ls.p) / absdot(ls.n, -w);
        if (isinf(pdf)) pdf = 0.f;
    }
}
// ---- InfiniteAreaLight with constant radiance: Lmap is a 1x1 MIPMap (lights/infinite.cpp, core/mipmap.h:245-274).
// sinf/cosf/acosf/atan2f of the reference (glibc) are matched by evaluating in double and rounding once.
PG_DEV V3 mat3_mul(const float *m, V3 w) {  // Transform::operator()(Vector3), transform.h:233-239
    return mk(m[0] * w.x + m[1] * w.y + m[2] * w.z, m[3] * w.x + m[4] * w.y + m[5] * w.z, m[6] * w.x + m[7] * w.y + m[8] * w.z);
}
PG_DEV Spec env_lookup(const DScene &sc, const PgLight &l, float s0_, float t0_) {  // Lmap->Lookup(st): width 0 -> triangle(0, st), mipmap.h:214-243
    return mip_triangle(sc, sc.images[l.env_image], 0, s0_, t0_);
}
PG_DEV Spec env_le(const DScene &sc, const PgLight &l, V3 rayD) {  // InfiniteAreaLight::Le, infinite.cpp:93-97
    V3 w = normalize(mat3_mul(l.w2l, rayD));
    return env_lookup(sc, l, spherical_phi(w) * PG_INV2PI, spherical_theta(w) * PG_INVPI);
}
// ProjectionLight::Projection (projection.cpp:79-91) and GonioPhotometricLight::Scale (goniometric.h:67-76); Lookup(st) of
// their maps is triangle(0, st) (mipmap.h:214-243 with width 0)
PG_DEV Spec light_projection(const DScene &sc, const PgLight &l, V3 w) {
    const V3 wl = mat3_mul(l.w2l, w);
    if (wl.z < l.hither) return sp(0);
    const V3 p = m4_point(l.proj, wl);
    if (!(p.x >= l.screen[0] && p.x <= l.screen[2] && p.y >= l.screen[1] && p.y <= l.screen[3])) return sp(0);
    if (l.env_image < 0) return sp(1);
    float ox = p.x - l.screen[0], oy = p.y - l.screen[1];  // Bounds2::Offset
    if (l.screen[2] > l.screen[0]) ox /= l.screen[2] - l.screen[0];
    if (l.screen[3] > l.screen[1]) oy /= l.screen[3] - l.screen[1];
    return env_lookup(sc, l, ox, oy);
}
PG_DEV Spec light_gonio_scale(const DScene &sc, const PgLight &l, V3 w) {
    V3 wp = normalize(mat3_mul(l.w2l, w));
    const float t = wp.y; wp.y = wp.z; wp.z = t;
    const float theta = spherical_theta(wp), phi = spherical_phi(wp);
    if (l.env_image < 0) return sp(1);
    return env_lookup(sc, l, phi * PG_INV2PI, theta * PG_INVPI);
}
PG_DEV float env_sample_1d(const float *func, const float *cdf, float funcInt, int n, float u, float &pdf, int *off) {  // sampling.h:72-89
    int size = n + 1, first = 0, len = size;
    while (len > 0) {
        int half = len >> 1, middle = first + half;
        if (cdf[middle] <= u) { first = middle + 1; len -= half + 1; } else len = half;
    }
    int offset = first - 1; offset = offset < 0 ? 0 : (offset > size - 2 ? size - 2 : offset);
    if (off) *off = offset;
    float du = u - cdf[offset];
    if ((cdf[offset + 1] - cdf[offset]) > 0) du /= (cdf[offset + 1] - cdf[offset]);
    pdf = (funcInt > 0) ? func[offset] / funcInt : 0;
    return (offset + du) / n;
}
PG_DEV float env_pdf_li(const DScene &sc, const PgLight &l, V3 w) {  // InfiniteAreaLight::Pdf_Li, infinite.cpp:127-135; Distribution2D::Pdf, sampling.h:135-141
    V3 wi = mat3_mul(l.w2l, w);
    float theta = spherical_theta(wi), phi = spherical_phi(wi);
    float sinTheta = pg_sinf(theta);
    if (sinTheta == 0) return 0;
    float p0 = phi * PG_INV2PI, p1 = theta * PG_INVPI;
    const int nu = l.env_nu, nv = l.env_nv;
    const float *tab = sc.envTables + l.env_table;
    int iu = (int)(p0 * nu); iu = iu < 0 ? 0 : (iu > nu - 1 ? nu - 1 : iu);
    int iv = (int)(p1 * nv); iv = iv < 0 ? 0 : (iv > nv - 1 ? nv - 1 : iv);
    const float *row = tab + (size_t)(2 * nu + 2) * iv, *marg = tab + (size_t)(2 * nu + 2) * nv;
    return (row[iu] / marg[2 * nv + 1]) / (2 * PG_PI * PG_PI * sinTheta);
}
// EXT: the scene has primitives or lights beyond triangles + area / delta lights (spheres, infinite lights); the plain
// instantiation keeps the common kernels at their register count
template <bool EXT>
PG_DEV Spec light_sample_li(const DScene &sc, const PgLight &light, V3 refp, V3 refErr, V3 refn, float u0, float u1, V3 &wi, float &pdf,
                            LightSample &ls) {
    if (EXT && light.type == PG_LIGHT_INFINITE) {  // InfiniteAreaLight::Sample_Li, infinite.cpp:99-125
        float pdf0, pdf1;
        int v;
        const int nu = light.env_nu, nv = light.env_nv;
        const float *tab = sc.envTables + light.env_table, *marg = tab + (size_t)(2 * nu + 2) * nv;
        float d1 = env_sample_1d(marg, marg + nv, marg[2 * nv + 1], nv, u1, pdf1, &v);  // Distribution2D::SampleContinuous, sampling.h:127-134
        const float *row = tab + (size_t)(2 * nu + 2) * v;
        float d0 = env_sample_1d(row, row + nu, row[2 * nu + 1], nu, u0, pdf0, nullptr);
        float mapPdf = pdf0 * pdf1;
        ls.n = mk(0, 0, 0); ls.pError = mk(0, 0, 0); ls.p = refp;
        pdf = 0;
        if (mapPdf == 0) return sp(0);
        float theta = d1 * PG_PI, phi = d0 * 2 * PG_PI;
        float sT, cT, sP, cP;
        pg_sincosf(theta, &sT, &cT);
        pg_sincosf(phi, &sP, &cP);
        float cosTheta = (float)cT, sinTheta = (float)sT, sinPhi = (float)sP, cosPhi = (float)cP;
        wi = mat3_mul(light.l2w, mk(sinTheta * cosPhi, sinTheta * sinPhi, cosTheta));
        pdf = mapPdf / (2 * PG_PI * PG_PI * sinTheta);
        if (sinTheta == 0) pdf = 0;
        ls.p = refp + wi * (2 * light.world_radius);
        return env_lookup(sc, light, d0, d1);
    }
    if (light.type != PG_LIGHT_AREA) {  // delta lights: point.cpp:43-52, spot.cpp:51-60, distant.cpp:50-60
        const Spec I = sp3(light.L[0], light.L[1], light.L[2]);
        const V3 pos = mk(light.pos[0], light.pos[1], light.pos[2]);
        ls.n = mk(0, 0, 0); ls.pError = mk(0, 0, 0);  // VisibilityTester end point: Interaction(p, time, mediumInterface)
        pdf = 1.f;
        if (light.type == PG_LIGHT_DISTANT) {
            wi = pos;  // wLight
            ls.p = refp + pos * (2 * light.world_radius);  // pOutside
            return I;
        }
        wi = normalize(pos - refp);
        ls.p = pos;
        const float d2 = lensq(pos - refp);
        if (light.type == PG_LIGHT_SPOT) return (I * spot_falloff(light, -wi)) / d2;
        if (EXT && light.type == PG_LIGHT_PROJECTION) return (I * light_projection(sc, light, -wi)) / d2;  // projection.cpp:71-77
        if (EXT && light.type == PG_LIGHT_GONIO) return (I * light_gonio_scale(sc, light, -wi)) / d2;     // goniometric.cpp:43-52
        return I / d2;
    }
    Tri t = load_tri(sc, light.prim);
    const bool quadric = EXT && (t.flags & PG_PRIM_SPHERE);
    if (quadric && sc.spheres[__float_as_int(t.p0.x)].shape == PG_SHAPE_SPHERE)
        ls = sphere_sample(sc.spheres[__float_as_int(t.p0.x)], refp, refErr, refn, u0, u1, pdf);
    else {
        if (quadric) ls = quadric_sample_area(sc.spheres[__float_as_int(t.p0.x)], u0, u1, pdf);
        else ls = tri_sample_area(sc, t, light.prim, light.area, u0, u1, pdf);
        area_to_solid_angle(refp, ls, pdf);
    }
    if (pdf == 0 || lensq(ls.p - refp) == 0) { pdf = 0; return sp(0); }
    wi = normalize(ls.p - refp);
    return (light.two_sided || dot(ls.n, -wi) > 0) ? sp3(light.L[0], light.L[1], light.L[2]) : sp(0);
}
// The light as the shading kernel first meets it: DScene::lightHot's record, fetched in one round trip.
struct LightHot { int type, prim, two_sided; float area; Spec L; Tri tri; };
PG_DEV LightHot load_light_hot(const DScene &sc, int lightNum) {
    const float4 *h = sc.lightHot + 5 * (size_t)lightNum;
    const float4 h0 = h[0], h1 = h[1], a = h[2], b = h[3], c = h[4];
    LightHot lh;
    lh.type = __float_as_int(h0.x); lh.prim = __float_as_int(h0.y); lh.two_sided = __float_as_int(h0.z); lh.area = h0.w;
    lh.L = sp3(h1.x, h1.y, h1.z);
    lh.tri.p0 = mk(a.x, a.y, a.z); lh.tri.p1 = mk(b.x, b.y, b.z); lh.tri.p2 = mk(c.x, c.y, c.z);
    lh.tri.flags = __float_as_uint(a.w); lh.tri.material = __float_as_int(b.w); lh.tri.light = __float_as_int(c.w);
    return lh;
}
// light_sample_li for a light whose hot record is at hand: a diffuse area light on a triangle -- the common case -- is sampled
// from the record alone; everything else goes through the general routine (same arithmetic either way)
template <bool EXT>
PG_DEV Spec light_sample_li_hot(const DScene &sc, const LightHot &lh, const PgLight &light, V3 refp, V3 refErr, V3 refn, float u0, float u1, V3 &wi,
                                float &pdf, LightSample &ls) {
    if (lh.type != PG_LIGHT_AREA || (lh.tri.flags & PG_PRIM_SPHERE)) return light_sample_li<EXT>(sc, light, refp, refErr, refn, u0, u1, wi, pdf, ls);
    ls = tri_sample_area(sc, lh.tri, lh.prim, lh.area, u0, u1, pdf);
    area_to_solid_angle(refp, ls, pdf);
    if (pdf == 0 || lensq(ls.p - refp) == 0) { pdf = 0; return sp(0); }
    wi = normalize(ls.p - refp);
    return (lh.two_sided || dot(ls.n, -wi) > 0) ? lh.L : sp(0);
}

// LightDistribution::Lookup (lightdistrib.cpp:68-82,135-149) -> table of one Distribution1D
PG_DEV const float *light_distribution(const DScene &sc, V3 p) {
    if (sc.lightStrategy != PG_LIGHTS_SPATIAL) return sc.distTable;
    V3 o = p - mk(sc.bmin[0], sc.bmin[1], sc.bmin[2]);  // Bounds3::Offset, geometry.h:801-807
    if (sc.bmax[0] > sc.bmin[0]) o.x /= sc.bmax[0] - sc.bmin[0];
    if (sc.bmax[1] > sc.bmin[1]) o.y /= sc.bmax[1] - sc.bmin[1];
    if (sc.bmax[2] > sc.bmin[2]) o.z /= sc.bmax[2] - sc.bmin[2];
    int pi0 = (int)(o.x * sc.nVoxels[0]), pi1 = (int)(o.y * sc.nVoxels[1]), pi2 = (int)(o.z * sc.nVoxels[2]);
    pi0 = pi0 < 0 ? 0 : (pi0 > sc.nVoxels[0] - 1 ? sc.nVoxels[0] - 1 : pi0);
    pi1 = pi1 < 0 ? 0 : (pi1 > sc.nVoxels[1] - 1 ? sc.nVoxels[1] - 1 : pi1);
    pi2 = pi2 < 0 ? 0 : (pi2 > sc.nVoxels[2] - 1 ? sc.nVoxels[2] - 1 : pi2);
    size_t idx = ((size_t)pi2 * sc.nVoxels[1] + pi1) * sc.nVoxels[0] + pi0;
    if (sc.sparseLights) {  // computed on first touch, like the reference's hash table: ask for it and let the caller retry
        const int slot = sc.voxelSlot[idx];
        if (slot >= 0) return sc.distTable + (size_t)slot * (size_t)(2 * sc.nLights + 2);
        if (slot == -1 && atomicCAS(&sc.voxelSlot[idx], -1, -2) == -1) sc.voxelRequests[atomicAdd(&sc.voxelCounters[0], 1)] = (int)idx;
        return nullptr;
    }
    return sc.distTable + idx * (size_t)(2 * sc.nLights + 2);
}

#endif  // PG_LIGHT_H
