// pg_lightdistrib.h -- SpatialLightDistribution::ComputeDistribution (lightdistrib.cpp:232-300) as device functions, once for the dense and the
// sparse table kernel: a voxel's world box, its sample points, one light's contribution at a sample point, and the sequential tail over the
// lights (sumContrib, minContrib, the Distribution1D constructor).  The lookup side of the same tables is light_distribution (pg_light.h).
//
// Used by k_light_tables and k_light_tables_sparse (pg_kernels.hip), which keep their loop nests: samples outside and lights inside with one
// lane per voxel, or the lights across a block with thread 0 running the tail.  Pinned on the host (tests/test_device_headers_on_host.py) and
// on the device (tests/test_gpu_device_arithmetic.py) through tests/film_probe.h.
#ifndef PG_LIGHTDISTRIB_H
#define PG_LIGHTDISTRIB_H
#include "pg_device.h"
#include "pg_kernels.h"
#include "pg_light.h"

#define PG_VOXEL_SAMPLES 128  // nSamples, lightdistrib.cpp:255

// World bounds of voxel v (x fastest) of the nVoxels grid over the scene's bounds, lightdistrib.cpp:238-247
PG_DEV void voxel_bounds(const int *nVoxels, const float *bmin, const float *bmax, int v, V3 &vmin, V3 &vmax) {
    int pi0 = v % nVoxels[0], pi1 = (v / nVoxels[0]) % nVoxels[1], pi2 = v / (nVoxels[0] * nVoxels[1]);
    V3 p0 = mk((float)pi0 / (float)nVoxels[0], (float)pi1 / (float)nVoxels[1], (float)pi2 / (float)nVoxels[2]);
    V3 p1 = mk((float)(pi0 + 1) / (float)nVoxels[0], (float)(pi1 + 1) / (float)nVoxels[1], (float)(pi2 + 1) / (float)nVoxels[2]);
    V3 a = mk(plerp(p0.x, bmin[0], bmax[0]), plerp(p0.y, bmin[1], bmax[1]), plerp(p0.z, bmin[2], bmax[2]));
    V3 b = mk(plerp(p1.x, bmin[0], bmax[0]), plerp(p1.y, bmin[1], bmax[1]), plerp(p1.z, bmin[2], bmax[2]));
    vmin = mk(pmin(a.x, b.x), pmin(a.y, b.y), pmin(a.z, b.z)); vmax = mk(pmax(a.x, b.x), pmax(a.y, b.y), pmax(a.z, b.z));
}
// Sample point i of a voxel: the point po and the pair (u0, u1) every light is sampled with there, lightdistrib.cpp:258-265
struct VoxelSample { V3 po; float u0, u1; };
PG_DEV VoxelSample voxel_sample(V3 vmin, V3 vmax, int i) {
    VoxelSample s;
    V3 t = mk(radical_inverse_base2(i), radical_inverse(3, i), radical_inverse(5, i));
    s.po = mk(plerp(t.x, vmin.x, vmax.x), plerp(t.y, vmin.y, vmax.y), plerp(t.z, vmin.z, vmax.z));
    s.u0 = radical_inverse(7, i); s.u1 = radical_inverse(11, i);
    return s;
}
// One light's sample at a sample point added to its lightContrib, lightdistrib.cpp:266-277: nothing without a pdf > 0
PG_DEV void voxel_light_contribution(const DScene &sc, const PgLight &light, const VoxelSample &s, float &lightContrib) {
    float pdf;
    V3 wi;
    LightSample ls;
    Spec Li = light_sample_li<true>(sc, light, s.po, mk(0, 0, 0), mk(0, 0, 0), s.u0, s.u1, wi, pdf, ls);  // Interaction(po, Normal3f(), Vector3f(), ...)
    if (pdf > 0) lightContrib += lum(Li) / pdf;
}
// func[0 .. nl) = lightContrib summed over nSamples points -> the voxel's Distribution1D in place: func clamped from below (lightdistrib.cpp:285-294),
// cdf[0 .. nl] behind it and funcInt at func[2 nl + 1] (sampling.h:57-70); every sum runs over the lights in order
PG_DEV void distribution_finish(float *func, float *cdf, int nl, int nSamples) {
    float sumContrib = 0;
    for (int j = 0; j < nl; ++j) sumContrib = sumContrib + func[j];
    float avgContrib = sumContrib / (float)((size_t)nSamples * (size_t)nl);
    float minContrib = (avgContrib > 0) ? (float)(.001 * (double)avgContrib) : 1.f;
    for (int j = 0; j < nl; ++j) func[j] = pmax(func[j], minContrib);
    cdf[0] = 0;
    for (int i = 1; i < nl + 1; ++i) cdf[i] = cdf[i - 1] + func[i - 1] / nl;
    float funcInt = cdf[nl];
    if (funcInt == 0) { for (int i = 1; i < nl + 1; ++i) cdf[i] = (float)i / (float)nl; }
    else { for (int i = 1; i < nl + 1; ++i) cdf[i] /= funcInt; }
    func[2 * nl + 1] = funcInt;
}

#endif  // PG_LIGHTDISTRIB_H
