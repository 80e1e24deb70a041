// render_check_host.hip -- pg_check_render_desc and the pure decisions of a frame (pbrt-v3_amd/csrc/pg_render_check.h) without a
// device: for every .pbrt file named on the command line, the front end's render description must be accepted; one hostile edit per
// check must be refused with the status and message pg_render reports; the batch shape and the bounce limits must be what
// pg_render has always computed.  No HIP call is made, so the program also runs under ASan / UBSan (tests/test_render_check.py
// builds it both ways).  Exit status 0: every expectation held.
#include <cstdio>
#include <cstring>
#include <string>
#include "pg_render_check.h"
#include "pbrt_host.h"

static int g_failures = 0, g_mutations = 0, g_checked = 0;

static void fail(const char *scene, const char *what, const std::string &detail) {
    fprintf(stderr, "FAIL %s: %s %s\n", scene, what, detail.c_str());
    ++g_failures;
}
static void refused(const char *scene, const char *what, const PgRenderDesc &rd, const RenderSceneFacts &f, const char *text) {
    std::string err;
    const int st = pg_check_render_desc(&rd, f, err);
    ++g_mutations;
    if (st != PG_ERR_INVALID || err.find(text) == std::string::npos)
        fail(scene, what, "-> status " + std::to_string(st) + " \"" + err + "\", expected " + std::to_string(PG_ERR_INVALID) + " \"" + text + "\"");
}

// one hostile edit per check of pg_render, on the scene that reaches it; the texts are those of pg_render before the checks moved
static void mutate(const char *scene, const std::string &name, const PgRenderDesc &rd, const RenderSceneFacts &f) {
    PgRenderDesc bad = rd;
    if (name == "cornell_32") {
        if (rd.filter_general || rd.sampler != PG_SAMPLER_HALTON) { fail(scene, "golden", "is not a Halton box-filter frame"); return; }
        bad.abi_version = PG_ABI_VERSION + 1;
        refused(scene, "abi_version", bad, f, ("ABI version " + std::to_string(PG_ABI_VERSION + 1) + ", expected " + std::to_string(PG_ABI_VERSION)).c_str());
        bad = rd; bad.filter_radius[1] = 0;
        refused(scene, "filter radius 0", bad, f, "pg_render: filter radius must be positive");
        bad = rd; bad.filter_radius[0] = 2.0f;  // test_unsupported_inputs_fail_loudly
        refused(scene, "wide box filter", bad, f, "pg_render: filter_general = 0 is the box filter of radius <= 0.5 with 256-entry tile blocks");
        bad = rd; bad.spp = 0;
        refused(scene, "spp 0", bad, f, "pg_render: bad spp/maxdepth/tile_step");
        bad = rd; bad.max_depth = -1;
        refused(scene, "maxdepth -1", bad, f, "pg_render: bad spp/maxdepth/tile_step");
        bad = rd; bad.max_depth = 1000;  // needs 8013 dimensions
        RenderSceneFacts g = f;
        if (g.nPermDims >= 1000) g.hasPerms = false;  // (a table that long serves any depth: then the scene without one)
        refused(scene, "Halton dimensions", bad, g, ("Halton table has " + std::to_string(f.nPermDims) + " dimensions; maxdepth 1000 needs 8013").c_str());
        bad = rd; bad.sampler = PG_SAMPLER_RANDOM;  // numbers up to OneMinusEpsilon round up from pixel 1 on
        refused(scene, "box filter that needs the gather", bad, f, "pg_render: filter_general = 0, but in this frame a film position can round up onto the next pixel "
                                                                   "(pg_box_filter_needs_gather, include/pbrt_gpu.h): render it with filter_general = 1");
    } else if (name == "filter_gaussian") {
        if (!rd.filter_general) { fail(scene, "golden", "is not a filter_general frame"); return; }
        bad.tile_pixels += 1;
        refused(scene, "tile_pixels", bad, f, "pg_render: tile_pixels does not match tile_halo");
    } else if (name == "vol_smoke") {  // test_invalid_media_and_sampler_descriptions_fail_loudly
        bad.camera_medium = f.nMedia;
        refused(scene, "camera_medium", bad, f, ("pg_render: camera_medium " + std::to_string(f.nMedia) + " out of range").c_str());
        bad = rd; bad.integrator = 2;
        refused(scene, "integrator 2", bad, f, "pg_render: integrator 2 (0 = path, 1 = volpath)");
        bad = rd; bad.sampler = 1; bad.sobol_resolution = 64; bad.sobol_log2_resolution = 6;
        refused(scene, "sobol without tables", bad, f, "pg_render: sampler = sobol, but the scene was created without the Sobol' tables");
    } else if (name == "sobol_cornell") {  // the same test's second half
        bad.sobol_resolution = 48;
        refused(scene, "sobol_resolution 48", bad, f, ("pg_render: sobol_resolution 48 / sobol_log2_resolution " + std::to_string(rd.sobol_log2_resolution)).c_str());
        bad = rd; bad.sampler = 7;
        refused(scene, "sampler 7", bad, f, "pg_render: sampler 7 (PgSamplerKind 0 .. 5)");
        bad = rd; bad.sampler = PG_SAMPLER_STRATIFIED; bad.strat_samples[0] = 3; bad.strat_samples[1] = 2;
        refused(scene, "strata", bad, f, ("pg_render: stratified sampler 3 x 2 samples, spp " + std::to_string(rd.spp)).c_str());
        bad = rd; bad.sampler = PG_SAMPLER_MAXMINDIST; bad.sampler_dims = 2;
        refused(scene, "maxmindist without cmaxmin", bad, f, "pg_render: maxmindist needs PgSceneDesc.cmaxmin, sampler_dims >= 1 and spp < 2^17");
    } else if (name == "sampler_stratified_dims") {
        bad.sampler_dims = 4097;
        refused(scene, "sampler_dims", bad, f, "pg_render: sampler_dims 4097");
    } else if (name == "sampler_maxmindist") {
        bad.spp = 3;
        refused(scene, "spp 3", bad, f, ("pg_render: sampler " + std::to_string(PG_SAMPLER_MAXMINDIST) + " needs a power-of-two spp (the reference rounds up), got 3").c_str());
    }
}

// Expected pairs computed by hand from pg_render's formula: more paths than the budget -> filter_general: tiles = max(1, budget / (256 spp)),
// all samples; box: samples = budget / (256 tiles), and if that is 0: one sample of max(1, budget / 256) tiles.
static void checkBatchShapes() {
    const size_t budgets[4] = {256, 768, 5000, (size_t)1 << 27};
    struct Case { int tiles, spp; int general[4][2], box[4][2]; };
    const Case cases[2] = {
        {6, 4, {{1, 4}, {1, 4}, {4, 4}, {6, 4}}, {{1, 1}, {3, 1}, {6, 3}, {6, 4}}},
        {8160, 64, {{1, 64}, {1, 64}, {1, 64}, {8160, 64}}, {{1, 1}, {3, 1}, {19, 1}, {8160, 64}}},  // (8160 x 256 x 64 = 133 693 440 <= 2^27)
    };
    for (const Case &c : cases)
        for (int b = 0; b < 4; ++b)
            for (int general = 0; general < 2; ++general) {
                const BatchShape s = pgBatchShape(c.spp, c.tiles, general != 0, budgets[b]);
                const int *want = general ? c.general[b] : c.box[b];
                const std::string what = std::to_string(c.tiles) + " tiles x " + std::to_string(c.spp) + " spp, budget " + std::to_string(budgets[b]) + (general ? ", general" : ", box");
                ++g_checked;
                if (s.tiles != want[0] || s.samples != want[1]) fail("batch shape", what.c_str(), "-> " + std::to_string(s.tiles) + " x " + std::to_string(s.samples));
                if (general && s.samples != c.spp) fail("batch shape", what.c_str(), "splits a tile's samples");
                if (!general && budgets[b] >= (size_t)c.tiles * 256 && s.tiles != c.tiles) fail("batch shape", what.c_str(), "does not take all tiles");
                if (s.tiles < 1 || s.samples < 1 || s.tiles > c.tiles || s.samples > c.spp) fail("batch shape", what.c_str(), "out of range");
            }
}
static void checkBounceLimits() {
    struct Case { int maxDepth; bool nullMat; long long want; int maxIters; };
    const Case cases[6] = {{5, false, 6, 6}, {5, true, 70, 70}, {100, false, 101, 101}, {100, true, 165, 165},
                           {2147483647, false, 2147483648LL, 4096}, {2147483647, true, 2147483712LL, 4096}};
    for (const Case &c : cases) {
        const BounceLimits l = pgBounceLimits(c.maxDepth, c.nullMat);
        ++g_checked;
        if (l.wantIters != c.want || l.maxIters != c.maxIters) fail("bounce limits", std::to_string(c.maxDepth).c_str(), "-> " + std::to_string(l.wantIters) + " / " + std::to_string(l.maxIters));
    }
    if (PG_MAX_BLIND_BOUNCES != 64 || PG_MAX_BOUNCES != 4096) fail("bounce limits", "constants", "changed");
}

int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) {
        const char *path = argv[a];
        PbrtHostScene *hs = pbrt_host_load_file(path, 0, nullptr);
        if (!hs) { fail(path, "pbrt_host_load_file", "returned no scene"); continue; }
        PreparedScene ps;
        std::string err;
        if (pg_prepare_scene(pbrt_host_scene_desc(hs), 11, ps, err) != PG_OK) { fail(path, "pg_prepare_scene", err); pbrt_host_free(hs); continue; }
        // what pg_render knows about the scene it renders on
        const RenderSceneFacts f = {ps.nMedia, ps.cmaxmin.p != nullptr, ps.sobolMatrices.p != nullptr, ps.perms.p != nullptr, ps.d.nPermDims};
        PgRenderDesc rd;
        pbrt_host_render_desc(hs, &rd);
        if (pg_check_render_desc(&rd, f, err) != PG_OK) fail(path, "the front end's description", "-> \"" + err + "\", expected PG_OK");
        if (pgTileCount(&rd) < 1) fail(path, "pgTileCount", "no tile");
        std::string name = path;
        name = name.substr(name.find_last_of('/') + 1);
        name = name.substr(0, name.find('.'));
        mutate(path, name, rd, f);
        pbrt_host_free(hs);
    }
    checkBatchShapes();
    checkBounceLimits();
    printf("render_check_host: %d scenes, %d hostile descriptions, %d decisions, %d failures\n", argc - 1, g_mutations, g_checked, g_failures);
    return g_failures == 0 ? 0 : 1;
}
