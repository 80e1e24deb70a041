// pg_render_check.h -- everything pg_render (pg_abi.hip) decides from the caller's PgRenderDesc before it touches the device: the checks
// of the description, in the order and with the texts they have always been reached, and the pure decisions of a frame (tile count,
// batch shape, bounce limits).  Host code only: no HIP runtime call, so a program without a device can run it
// (tests/render_check_host.hip does, under the sanitizers).
#ifndef PG_RENDER_CHECK_H
#define PG_RENDER_CHECK_H
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include "pg_scene_prep.h"  // pgPrepFail
// What the checks need to know about the scene the frame is rendered on
struct RenderSceneFacts {
    int nMedia = 0;                                               // PgSceneDesc.n_media
    bool hasCmaxmin = false, hasSobol = false, hasPerms = false;  // the scene carries CMaxMinDist / the Sobol' matrices / the Halton permutations
    int nPermDims = 0;                                            // dimensions of the Halton permutation table
    // pg_check_direct_desc alone:
    int nLights = 0;                                              // PgSceneDesc.n_lights
    bool maySpecularLobes = false;                                // pgh_scene_may_add_specular_lobes(the scene's description)
};
// the 16x16 tiles of the full-frame tiling that this description's shard (tile_first, tile_step) owns
inline int pgTileCount(const PgRenderDesc *rd) {
    int nx = (rd->sample_bounds[2] - rd->sample_bounds[0] + 15) / 16, ny = (rd->sample_bounds[3] - rd->sample_bounds[1] + 15) / 16;
    if (nx <= 0 || ny <= 0 || rd->tile_step <= 0 || rd->tile_first < 0) return 0;
    int total = nx * ny;
    return rd->tile_first >= total ? 0 : (total - rd->tile_first + rd->tile_step - 1) / rd->tile_step;
}

// ABI 30 appended to PgRenderDesc (the realistic camera's lens block) and to PgCounters (its two statistics) and changed nothing before them; PgSceneDesc is
// the same.  A caller compiled against ABI 29 -- a host application, or the reference-side binding, built before the library was replaced -- therefore goes on
// working: its descriptions are taken as what they are, the first PG_ABI29_RENDER_DESC_BYTES of today's PgRenderDesc with the lens block absent (no byte behind
// them is read), and pg_counters fills the PG_ABI29_COUNTERS_BYTES such a caller has room for.  Any other version is refused as before.
#define PG_ABI_OLDEST_ACCEPTED 29
#define PG_ABI29_RENDER_DESC_BYTES offsetof(PgRenderDesc, n_lens_interfaces)
#define PG_ABI29_COUNTERS_BYTES offsetof(PgCounters, lens_rays_total)
inline bool pgAbiAccepted(int version) { return version >= PG_ABI_OLDEST_ACCEPTED && version <= PG_ABI_VERSION; }
// The caller's render description as a description of THIS version: `rd` itself, or -- for an ABI 29 caller -- `local`, filled from the bytes that caller owns
// (an ABI 29 caller's object is SHORTER than PgRenderDesc: until the version is known the description is read as bytes, never through a member of the longer type)
inline const PgRenderDesc *pgCurrentRenderDesc(const PgRenderDesc *rd, PgRenderDesc &local) {
    static_assert(offsetof(PgRenderDesc, abi_version) == 0, "the version is a description's first field");
    int32_t version;
    memcpy(&version, rd, sizeof(version));
    if (version != 29) return rd;
    memset(&local, 0, sizeof(local));
    memcpy(&local, rd, PG_ABI29_RENDER_DESC_BYTES);
    local.abi_version = PG_ABI_VERSION;
    return &local;
}

// PG_OK, or PG_ERR_INVALID with its message in err
#define RC_FAIL(...) return pgPrepFail(err, PG_ERR_INVALID, __VA_ARGS__)
inline int pg_check_render_desc(const PgRenderDesc *rd, const RenderSceneFacts &sc, std::string &err) {
    if (rd->abi_version != PG_ABI_VERSION) RC_FAIL("ABI version %d, expected %d", rd->abi_version, PG_ABI_VERSION);
    if (rd->filter_radius[0] <= 0 || rd->filter_radius[1] <= 0) RC_FAIL("pg_render: filter radius must be positive");
    if (!rd->filter_general && (rd->filter_radius[0] > 0.5f || rd->filter_radius[1] > 0.5f || rd->tile_pixels != 256))
        RC_FAIL("pg_render: filter_general = 0 is the box filter of radius <= 0.5 with 256-entry tile blocks");
    if (rd->filter_general && rd->tile_pixels != (16 + rd->tile_halo[0] + rd->tile_halo[2]) * (16 + rd->tile_halo[1] + rd->tile_halo[3]))
        RC_FAIL("pg_render: tile_pixels does not match tile_halo");
    if (rd->spp <= 0 || rd->max_depth < 0 || rd->tile_step <= 0) RC_FAIL("pg_render: bad spp/maxdepth/tile_step");
    if (rd->integrator != 0 && rd->integrator != 1) RC_FAIL("pg_render: integrator %d (0 = path, 1 = volpath)", rd->integrator);
    if (rd->camera_medium < -1 || rd->camera_medium >= sc.nMedia) RC_FAIL("pg_render: camera_medium %d out of range", rd->camera_medium);
    if (rd->sampler < PG_SAMPLER_HALTON || rd->sampler > PG_SAMPLER_MAXMINDIST) RC_FAIL("pg_render: sampler %d (PgSamplerKind 0 .. 5)", rd->sampler);
    if (rd->sampler >= PG_SAMPLER_RANDOM) {
        if (rd->sampler != PG_SAMPLER_RANDOM && (rd->sampler_dims < 0 || rd->sampler_dims > 4096)) RC_FAIL("pg_render: sampler_dims %d", rd->sampler_dims);
        if (rd->sampler == PG_SAMPLER_STRATIFIED && (rd->strat_samples[0] < 1 || rd->strat_samples[1] < 1 || rd->strat_samples[0] * rd->strat_samples[1] != rd->spp))
            RC_FAIL("pg_render: stratified sampler %d x %d samples, spp %d", rd->strat_samples[0], rd->strat_samples[1], rd->spp);
        if ((rd->sampler == PG_SAMPLER_ZEROTWO || rd->sampler == PG_SAMPLER_MAXMINDIST) && (rd->spp & (rd->spp - 1)))
            RC_FAIL("pg_render: sampler %d needs a power-of-two spp (the reference rounds up), got %d", rd->sampler, rd->spp);
        if (rd->sampler == PG_SAMPLER_MAXMINDIST && (!sc.hasCmaxmin || rd->sampler_dims < 1 || rd->spp >= (1 << 17)))
            RC_FAIL("pg_render: maxmindist needs PgSceneDesc.cmaxmin, sampler_dims >= 1 and spp < 2^17");
    }
    if (rd->sampler == 1) {
        if (!sc.hasSobol) RC_FAIL("pg_render: sampler = sobol, but the scene was created without the Sobol' tables");
        if (rd->sobol_log2_resolution < 0 || rd->sobol_log2_resolution > 26 || rd->sobol_resolution != (1 << rd->sobol_log2_resolution))
            RC_FAIL("pg_render: sobol_resolution %d / sobol_log2_resolution %d", rd->sobol_resolution, rd->sobol_log2_resolution);
    }
    if (rd->sampler == 0 && (!sc.hasPerms || (5 + 8 * ((long long)rd->max_depth + 1) > sc.nPermDims && sc.nPermDims < 1000)))
        RC_FAIL("Halton table has %d dimensions; maxdepth %d needs %lld", sc.nPermDims, rd->max_depth, 5 + 8 * ((long long)rd->max_depth + 1));
    if (!rd->filter_general && pgh_box_filter_needs_gather(rd))
        RC_FAIL("pg_render: filter_general = 0, but in this frame a film position can round up onto the next pixel "
                "(pg_box_filter_needs_gather, include/pbrt_gpu.h): render it with filter_general = 1");
    // ABI 30: the cameras, and the realistic camera's lens block (the device indexes both tables with what is checked here)
    if (rd->camera_type < 0 || rd->camera_type > 3) RC_FAIL("pg_render: camera_type %d (0 = perspective, 1 = orthographic, 2 = environment, 3 = realistic)", rd->camera_type);
    if (rd->camera_type == 3) {
        if (rd->n_lens_interfaces < 1 || rd->n_lens_interfaces > PG_MAX_LENS_INTERFACES)
            RC_FAIL("pg_render: realistic camera with %d lens interfaces (1 .. %d)", rd->n_lens_interfaces, PG_MAX_LENS_INTERFACES);
        for (int i = 0; i < rd->n_lens_interfaces; ++i)
            if (!(rd->lens_interfaces[i][3] > 0) || !std::isfinite(rd->lens_interfaces[i][3]))
                RC_FAIL("pg_render: lens interface %d has aperture radius %g (finite and positive)", i, (double)rd->lens_interfaces[i][3]);
        for (int i = 0; i < 64; ++i)
            if (!(rd->exit_pupil_bounds[i][0] <= rd->exit_pupil_bounds[i][2] && rd->exit_pupil_bounds[i][1] <= rd->exit_pupil_bounds[i][3]))
                RC_FAIL("pg_render: exit pupil box %d is empty (min > max)", i);
        if (!(rd->film_diagonal > 0) || !std::isfinite(rd->film_diagonal)) RC_FAIL("pg_render: realistic camera on a film of diagonal %g", (double)rd->film_diagonal);
    }
    return PG_OK;
}
// The DirectLightingIntegrator's description beside a frame's (pg_render_direct): called once pg_check_render_desc has passed `rd`.
// The reference's own limits on a GlobalSampler's dimensions: halton.h:71-76 (PrimeTableSize, lowdiscrepancy.h:52) and sobol.cpp:47-50
// (NumSobolDimensions, sobolmatrices.h:46) end its process beyond them.
const long long PG_HALTON_MAX_DIMS = 1000, PG_SOBOL_MAX_DIMS = 1024;
inline int pg_check_direct_desc(const PgRenderDesc *rd, const PgDirectLightingDesc *dl, const RenderSceneFacts &sc, std::string &err) {
    if (dl->strategy != 0 && dl->strategy != 1) RC_FAIL("pg_render_direct: strategy %d (0 = all, 1 = one)", dl->strategy);
    if (dl->n_lights != sc.nLights) RC_FAIL("pg_render_direct: n_lights %d, the scene has %d lights", dl->n_lights, sc.nLights);
    if (dl->strategy == 0) {
        if (dl->n_lights > 0 && !dl->light_samples) RC_FAIL("pg_render_direct: strategy 0 (all) needs light_samples, one count per light");
        for (int j = 0; j < dl->n_lights; ++j)
            if (dl->light_samples[j] < 1) RC_FAIL("pg_render_direct: light_samples[%d] = %d (each light takes at least one sample)", j, dl->light_samples[j]);
    }
    if (rd->integrator != 0) RC_FAIL("pg_render_direct: integrator %d (the frame's description carries 0 here; max_depth is the integrator's \"maxdepth\")", rd->integrator);
    // UniformSampleAllLights reads sample ARRAYS (integrator.cpp:61-64).  A GlobalSampler's are closed form per element (sampler.cpp:136-166); a
    // PixelSampler fills them from its tile's RNG stream in StartPixel (stratified.cpp:62-69, zerotwosequence.cpp:62-68, maxmin.cpp:65-75)
    if (dl->strategy == 0 && rd->sampler >= PG_SAMPLER_RANDOM)
        RC_FAIL("pg_render_direct: strategy 0 (all) under sampler %d: the PixelSamplers' sample arrays are not built (render with halton or sobol, or with strategy 1)", rd->sampler);
    // directlighting.cpp:91-95: SpecularReflect + SpecularTransmit while depth + 1 < maxDepth -- a depth-first tree that is not built
    if (rd->max_depth >= 2 && sc.maySpecularLobes)
        RC_FAIL("pg_render_direct: maxdepth %d on a scene whose materials can add specular lobes: directlighting's specular bounces are not built (maxdepth <= 1 renders such a scene)", rd->max_depth);
    if (rd->sampler == PG_SAMPLER_HALTON || rd->sampler == PG_SAMPLER_SOBOL) {
        // Dimensions 0 .. 4 are the camera sample's.  Strategy 0 with max_depth >= 1: the constructor requested two arrays per light and depth
        // (directlighting.cpp:53-60), which occupy 5 .. 5 + 4 n_lights max_depth -- StartPixel computes them all -- and those of depth 0 are read;
        // otherwise the draws are sequential from 5: lightNum, uLight, uScattering (strategy 1), or uLight, uScattering per light (max_depth 0)
        const bool arrays = dl->strategy == 0 && rd->max_depth >= 1;
        const long long reached = arrays ? 5 + 4 * (long long)dl->n_lights * rd->max_depth : (dl->strategy == 1 ? 5 + 5 : 5 + 4 * (long long)dl->n_lights);
        const long long read = dl->strategy == 1 ? 5 + 5 : 5 + 4 * (long long)dl->n_lights;
        const long long limit = rd->sampler == PG_SAMPLER_HALTON ? PG_HALTON_MAX_DIMS : PG_SOBOL_MAX_DIMS;
        if (dl->n_lights > 0 && reached > limit)
            RC_FAIL("pg_render_direct: the frame reaches sample dimension %lld; the reference's %s ends at %lld (it aborts beyond)", reached, rd->sampler == PG_SAMPLER_HALTON ? "Halton sampler" : "Sobol' sampler", limit);
        if (dl->n_lights > 0 && rd->sampler == PG_SAMPLER_HALTON && read > sc.nPermDims)
            RC_FAIL("pg_render_direct: Halton table has %d dimensions; %d lights under strategy %d need %lld", sc.nPermDims, dl->n_lights, dl->strategy, read);
    }
    return PG_OK;
}
#undef RC_FAIL
// Batch shape: as many whole tiles x samples as fit the budget of path slots
struct BatchShape { int tiles, samples; };
inline BatchShape pgBatchShape(int spp, int nLocalTiles, bool filterGeneral, size_t budget) {
    BatchShape b = {nLocalTiles, spp};
    if ((size_t)b.tiles * 256 * b.samples <= budget) return b;
    if (filterGeneral) {
        // the gathering film kernel needs all samples of a tile in one batch (reference summation order): split by tiles
        b.tiles = std::max(1, (int)(budget / ((size_t)256 * b.samples)));
    } else {
        // prefer all tiles with fewer samples (keeps primary rays coherent and every pixel busy)
        b.samples = (int)(budget / ((size_t)b.tiles * 256));
        if (b.samples < 1) { b.samples = 1; b.tiles = std::max(1, (int)(budget / 256)); }
    }
    return b;
}

// (64-bit: maxdepth comes from the caller / the scene file.)  Bounce launches are enqueued without looking at the queues, so
// a huge maxdepth is bounded here: beyond PG_MAX_BLIND_BOUNCES the host looks at the main queue every 32 bounces and stops
// when it is empty (Russian roulette ends every path), and a frame whose paths outlive PG_MAX_BOUNCES fails loudly.
const long long PG_MAX_BLIND_BOUNCES = 64, PG_MAX_BOUNCES = 4096;
struct BounceLimits { long long wantIters; int maxIters; };
inline BounceLimits pgBounceLimits(int maxDepth, bool hasNullMaterial) {
    const long long want = (long long)maxDepth + 1 + (hasNullMaterial ? 64 : 0);
    return {want, (int)std::min<long long>(want, PG_MAX_BOUNCES)};
}
#endif
