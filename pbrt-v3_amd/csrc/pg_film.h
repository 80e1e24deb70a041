// pg_film.h -- SamplerIntegrator::Render's sample scrub (integrator.cpp:294-315) and FilmTile::AddSample (film.h:121-161, the tile of
// film.cpp:95-106) as device functions, once for the three film kernels: a tile's sample and pixel bounds, the radiance a sample adds,
// the pixels its filter footprint covers, the filter-table weight, the weighted contribution and the stray-sample record.
//
// Used by k_film, k_film_general and k_ts_film (pg_kernels.hip), which keep what differs between them: who owns which pixel, the loop order,
// where the sums are held, atomics versus gather.  Pinned on the host (tests/test_device_headers_on_host.py) and on the device
// (tests/test_gpu_device_arithmetic.py) through tests/film_probe.h.
#ifndef PG_FILM_H
#define PG_FILM_H
#include "pg_device.h"
#include "pg_kernels.h"

// Tile `local` of the shard: its samples' pixels [x0, x1) x [y0, y1) and the FilmTile's pixel bounds [tp0, tp1), film.cpp:95-106
struct FilmTileBounds { int x0, y0, x1, y1, tp0x, tp0y, tp1x, tp1y; };
PG_DEV FilmTileBounds film_tile_bounds(const PgRenderDesc &rd, int nTilesX, int local) {
    FilmTileBounds b;
    const int t = rd.tile_first + local * rd.tile_step;
    const int tx = t % nTilesX, ty = t / nTilesX;
    b.x0 = rd.sample_bounds[0] + tx * 16; b.y0 = rd.sample_bounds[1] + ty * 16;
    b.x1 = min(b.x0 + 16, rd.sample_bounds[2]); b.y1 = min(b.y0 + 16, rd.sample_bounds[3]);
    const float frx = rd.filter_radius[0], fry = rd.filter_radius[1];
    b.tp0x = max((int)ceilf((float)b.x0 - 0.5f - frx), rd.cropped_pixel_bounds[0]);
    b.tp0y = max((int)ceilf((float)b.y0 - 0.5f - fry), rd.cropped_pixel_bounds[1]);
    b.tp1x = min((int)floorf((float)b.x1 - 0.5f + frx) + 1, rd.cropped_pixel_bounds[2]);
    b.tp1y = min((int)floorf((float)b.y1 - 0.5f + fry) + 1, rd.cropped_pixel_bounds[3]);
    return b;
}
// filter_general: a tile's film block is its 16 x 16 pixels with the halo around them, row-major from (bx0, by0), tw pixels wide
struct FilmBlock { int tw, bx0, by0; };
PG_DEV FilmBlock film_block(const PgRenderDesc &rd, const FilmTileBounds &b) {
    FilmBlock k;
    k.tw = 16 + rd.tile_halo[0] + rd.tile_halo[2];
    k.bx0 = b.x0 - rd.tile_halo[0]; k.by0 = b.y0 - rd.tile_halo[1];
    return k;
}
// What Render hands to AddSample for the radiance Li returned (integrator.cpp:294-315), then AddSample's clamp (film.h:124-125)
PG_DEV Spec film_sample_radiance(const PgRenderDesc &rd, Spec L) {
    if (isnan(L.r) || isnan(L.g) || isnan(L.b)) L = sp(0);
    else if ((double)lum(L) < -1e-5) L = sp(0);
    else if (isinf(lum(L))) L = sp(0);
    if (lum(L) > rd.max_sample_luminance) L = L * (rd.max_sample_luminance / lum(L));
    return L;
}
// The pixels [p0, p1) of one axis a sample at d = pFilm - 0.5 (pFilmDiscrete) covers with filter radius r, within the tile's [tp0, tp1): film.h:126-132
PG_DEV void film_footprint_axis(float d, float r, int tp0, int tp1, int &p0, int &p1) {
    p0 = max((int)ceilf(d - r), tp0);
    p1 = min((int)floorf(d + r) + 1, tp1);
}
PG_DEV void film_footprint(float dx, float dy, float frx, float fry, const FilmTileBounds &b, int &p0x, int &p0y, int &p1x, int &p1y) {
    film_footprint_axis(dx, frx, b.tp0x, b.tp1x, p0x, p1x);
    film_footprint_axis(dy, fry, b.tp0y, b.tp1y, p0y, p1y);
}
// filterTable[ify[y] * filterTableSize + ifx[x]] for pixel (X, Y), film.h:137-154; invR = FilmTile::invFilterRadius, film.h:113
PG_DEV float film_filter_weight(const PgRenderDesc &rd, int X, int Y, float dx, float dy, float invRx, float invRy) {
    const float fx = fabsf(((float)X - dx) * invRx * 16), fy = fabsf(((float)Y - dy) * invRy * 16);
    const int ifx = min((int)floorf(fx), 15), ify = min((int)floorf(fy), 15);
    return rd.filter_table[ify * 16 + ifx];
}
// sampleWeight: Camera::GenerateRayDifferential's return value -- the realistic camera's frames (WEIGHTED) keep it in the LensFrame; the other
// cameras' is 1 and their kernels do not read one
template <bool WEIGHTED>
PG_DEV float film_sample_weight(const PathState &st, int slot) { return WEIGHTED ? lens_frame(st.L)->weights[slot] : 1.f; }
// pixel.contribSum += L * sampleWeight * filterWeight, film.h:158
PG_DEV Spec film_contribution(Spec L, float sampleWeight, float filterWeight) { return (L * sampleWeight) * filterWeight; }
// A box-filter sample of pixel (px, py) that covers another pixel (x, y): recorded for the host, which adds it in the reference's order
PG_DEV void film_stray_append(PgStraySample *strays, int maxStrays, int *nStrays, int x, int y, int px, int py, Spec c) {
    const int k = atomicAdd(nStrays, 1);
    if (k < maxStrays) {
        PgStraySample s;
        s.px = x; s.py = y; s.src_px = px; s.src_py = py;
        s.rgb[0] = c.r; s.rgb[1] = c.g; s.rgb[2] = c.b; s.weight = 1.f;
        strays[k] = s;
    }
}

#endif  // PG_FILM_H
