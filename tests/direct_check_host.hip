// direct_check_host.hip -- pg_check_direct_desc (pbrt-v3_amd/csrc/pg_render_check.h), what pg_render_direct decides from the caller's
// PgDirectLightingDesc before it touches the device, without a device: the fixtures of tests/golden/directlighting named on the command
// line are loaded by the front end, whose two descriptions must be accepted; one hostile edit per refusal must come back as
// PG_ERR_INVALID with its exact text.  No HIP call is made, so the program also runs under ASan / UBSan
// (tests/test_directlighting_check.py builds it both ways).  Exit status 0: every expectation held.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "pg_render_check.h"
#include "pbrt_host.h"

static int g_failures = 0, g_refusals = 0, g_accepted = 0;

static void fail(const std::string &scene, const char *what, const std::string &detail) {
    fprintf(stderr, "FAIL %s: %s %s\n", scene.c_str(), what, detail.c_str());
    ++g_failures;
}
static void refused(const std::string &scene, const char *what, const PgRenderDesc &rd, const PgDirectLightingDesc &dl, const RenderSceneFacts &f, const std::string &text) {
    std::string err;
    const int st = pg_check_direct_desc(&rd, &dl, f, err);
    ++g_refusals;
    if (st != PG_ERR_INVALID || err != text) fail(scene, what, "-> status " + std::to_string(st) + " \"" + err + "\", expected " + std::to_string(PG_ERR_INVALID) + " \"" + text + "\"");
}
static void accepted(const std::string &scene, const char *what, const PgRenderDesc &rd, const PgDirectLightingDesc &dl, const RenderSceneFacts &f) {
    std::string err;
    ++g_accepted;
    if (pg_check_render_desc(&rd, f, err) != PG_OK) fail(scene, what, "pg_check_render_desc -> \"" + err + "\"");
    else if (pg_check_direct_desc(&rd, &dl, f, err) != PG_OK) fail(scene, what, "-> \"" + err + "\", expected PG_OK");
}

struct Loaded { PbrtHostScene *hs; PgRenderDesc rd; PgDirectLightingDesc dl; RenderSceneFacts f; };

int main(int argc, char **argv) {
    std::map<std::string, Loaded> scenes;
    for (int a = 1; a < argc; ++a) {
        std::string name = argv[a];
        name = name.substr(name.find_last_of('/') + 1);
        name = name.substr(0, name.find('.'));
        Loaded l;
        l.hs = pbrt_host_load_file(argv[a], 0, nullptr);
        if (!l.hs) { fail(name, "pbrt_host_load_file", "returned no scene"); continue; }
        const PgSceneDesc *sd = pbrt_host_scene_desc(l.hs);
        PreparedScene ps;
        std::string err;
        if (pg_prepare_scene(sd, 11, ps, err) != PG_OK) { fail(name, "pg_prepare_scene", err); pbrt_host_free(l.hs); continue; }
        l.f = RenderSceneFacts{ps.nMedia, ps.cmaxmin.p != nullptr, ps.sobolMatrices.p != nullptr, ps.perms.p != nullptr, ps.d.nPermDims};
        l.f.nLights = sd->n_lights; l.f.maySpecularLobes = pgh_scene_may_add_specular_lobes(sd) != 0;  // what pg_render_direct knows about its scene
        pbrt_host_render_desc(l.hs, &l.rd);
        const PgDirectLightingDesc *dl = pbrt_host_direct_desc(l.hs);
        if (!dl) { fail(name, "pbrt_host_direct_desc", "is null for a directlighting scene"); pbrt_host_free(l.hs); continue; }
        l.dl = *dl;
        accepted(name, "the front end's descriptions", l.rd, l.dl, l.f);
        scenes[name] = l;
    }
    for (const char *need : {"a_defaults", "c_three_samples_sobol", "d_one_of_18", "h_specular_depth_1", "i_depth_0", "l2_one_stratified"})
        if (!scenes.count(need)) fail(need, "fixture", "not loaded");
    if (g_failures == 0) {
        const Loaded &a = scenes["a_defaults"], &c = scenes["c_three_samples_sobol"], &d = scenes["d_one_of_18"], &h = scenes["h_specular_depth_1"], &l2 = scenes["l2_one_stratified"];
        if (a.dl.strategy != 0 || a.dl.n_lights != 2 || a.rd.max_depth != 5 || a.f.maySpecularLobes) fail("a_defaults", "fixture", "is not the all-matte default frame");
        if (d.dl.strategy != 1 || d.dl.n_lights != 18) fail("d_one_of_18", "fixture", "is not strategy one over 18 lights");
        if (!h.f.maySpecularLobes || h.rd.max_depth != 1) fail("h_specular_depth_1", "fixture", "has no specular lobes at maxdepth 1");
        PgRenderDesc rd = a.rd;
        PgDirectLightingDesc dl = a.dl;
        dl.strategy = 2;
        refused("a_defaults", "strategy 2", rd, dl, a.f, "pg_render_direct: strategy 2 (0 = all, 1 = one)");
        dl = a.dl; dl.strategy = -1;
        refused("a_defaults", "strategy -1", rd, dl, a.f, "pg_render_direct: strategy -1 (0 = all, 1 = one)");
        dl = a.dl; dl.n_lights = 3;
        refused("a_defaults", "n_lights 3", rd, dl, a.f, "pg_render_direct: n_lights 3, the scene has 2 lights");
        dl = a.dl; dl.light_samples = nullptr;
        refused("a_defaults", "null light_samples", rd, dl, a.f, "pg_render_direct: strategy 0 (all) needs light_samples, one count per light");
        const int32_t zero[2] = {1, 0}, negative[2] = {-4, 1};
        dl = a.dl; dl.light_samples = zero;
        refused("a_defaults", "light_samples 0", rd, dl, a.f, "pg_render_direct: light_samples[1] = 0 (each light takes at least one sample)");
        dl = a.dl; dl.light_samples = negative;
        refused("a_defaults", "light_samples -4", rd, dl, a.f, "pg_render_direct: light_samples[0] = -4 (each light takes at least one sample)");
        dl = a.dl; rd = a.rd; rd.integrator = 1;
        refused("a_defaults", "integrator 1", rd, dl, a.f, "pg_render_direct: integrator 1 (the frame's description carries 0 here; max_depth is the integrator's \"maxdepth\")");
        // strategy 0 under each PixelSampler (the stratified frame's description with the sampler kind changed)
        for (int kind = PG_SAMPLER_RANDOM; kind <= PG_SAMPLER_MAXMINDIST; ++kind) {
            rd = l2.rd; rd.sampler = kind; dl = l2.dl; dl.strategy = 0;
            refused("l2_one_stratified", "strategy all under a PixelSampler", rd, dl, l2.f,
                    "pg_render_direct: strategy 0 (all) under sampler " + std::to_string(kind) + ": the PixelSamplers' sample arrays are not built (render with halton or sobol, or with strategy 1)");
        }
        rd = h.rd; rd.max_depth = 2;
        refused("h_specular_depth_1", "maxdepth 2", rd, h.dl, h.f,
                "pg_render_direct: maxdepth 2 on a scene whose materials can add specular lobes: directlighting's specular bounces are not built (maxdepth <= 1 renders such a scene)");
        rd = h.rd; rd.max_depth = 5; dl = h.dl; dl.strategy = 1;
        refused("h_specular_depth_1", "maxdepth 5, strategy one", rd, dl, h.f,
                "pg_render_direct: maxdepth 5 on a scene whose materials can add specular lobes: directlighting's specular bounces are not built (maxdepth <= 1 renders such a scene)");
        // sample dimensions: 60 lights at maxdepth 5 occupy 5 + 4 * 60 * 5 = 1205 dimensions, beyond both samplers' tables
        std::vector<int32_t> ones(60, 1);
        RenderSceneFacts many = a.f;
        many.nLights = 60;
        dl = a.dl; dl.n_lights = 60; dl.light_samples = ones.data();
        refused("a_defaults", "Halton beyond 1000", a.rd, dl, many, "pg_render_direct: the frame reaches sample dimension 1205; the reference's Halton sampler ends at 1000 (it aborts beyond)");
        many = c.f; many.nLights = 60;
        dl = c.dl; dl.n_lights = 60; dl.light_samples = ones.data();
        refused("c_three_samples_sobol", "Sobol' beyond 1024", c.rd, dl, many, "pg_render_direct: the frame reaches sample dimension 1205; the reference's Sobol' sampler ends at 1024 (it aborts beyond)");
        RenderSceneFacts shortTable = a.f;
        shortTable.nPermDims = 10;  // two lights read dimensions 5 .. 12
        refused("a_defaults", "short Halton table", a.rd, a.dl, shortTable, "pg_render_direct: Halton table has 10 dimensions; 2 lights under strategy 0 need 13");
        shortTable = d.f; shortTable.nPermDims = 9;  // strategy one reads dimensions 5 .. 9
        refused("d_one_of_18", "short Halton table, strategy one", d.rd, d.dl, shortTable, "pg_render_direct: Halton table has 9 dimensions; 18 lights under strategy 1 need 10");
        // accepted: the same edits on the other side of each line
        rd = h.rd; rd.max_depth = 0;
        accepted("h_specular_depth_1", "maxdepth 0", rd, h.dl, h.f);
        rd = a.rd; rd.max_depth = 2;
        accepted("a_defaults", "maxdepth 2 without specular lobes", rd, a.dl, a.f);
        dl = l2.dl;
        accepted("l2_one_stratified", "strategy one under a PixelSampler", l2.rd, dl, l2.f);
        many = a.f; many.nLights = 49; many.nPermDims = 1000;  // 5 + 4 * 49 * 5 = 985
        std::vector<int32_t> ones49(49, 1);
        dl = a.dl; dl.n_lights = 49; dl.light_samples = ones49.data();
        accepted("a_defaults", "985 dimensions", a.rd, dl, many);
    }
    for (auto &kv : scenes) pbrt_host_free(kv.second.hs);
    printf("direct_check_host: %d scenes, %d refusals, %d accepted, %d failures\n", (int)scenes.size(), g_refusals, g_accepted, g_failures);
    return g_failures == 0 ? 0 : 1;
}
