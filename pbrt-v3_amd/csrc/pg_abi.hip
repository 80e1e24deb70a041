// pg_abi.hip -- the C ABI of include/pbrt_gpu.h: scene upload, the wavefront
// render loop (SamplerIntegrator::Render, integrator.cpp:228-339, re-ordered
// into batches of camera samples that advance one bounce per launch), and the
// batched Scene::Intersect/IntersectP entry points.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <dlfcn.h>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "pg_device.h"
#include "pg_kernels.h"
#include "pg_scene_prep.h"
#include "pg_render_check.h"

static thread_local std::string g_lastError;
static int setError(int code, const char *fmt, ...) {
    char buf[1024];
    va_list a;
    va_start(a, fmt);
    vsnprintf(buf, sizeof(buf), fmt, a);
    va_end(a);
    g_lastError = buf;
    return code;
}
// for the other translation units of this library (pg_hlbvh.hip)
int pgSetError(int code, const char *msg) { g_lastError = msg; return code; }
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return setError(PG_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_));    \
    } while (0)

struct DeviceBuffer {
    void *p = nullptr;
    size_t bytes = 0;
    hipError_t alloc(size_t n) {
        release();
        bytes = n;
        if (n == 0) return hipSuccess;
        return hipMalloc(&p, n);
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    ~DeviceBuffer() { release(); }
};

struct PgScene {
    int device = 0;
    int callerAbi = PG_ABI_VERSION;  // the version the scene's creator was compiled against (pg_render_check.h): pg_counters fills what that caller's PgCounters holds
    DScene d;
    TraceConfig trace;  // k_trace's tunables for THIS scene's launches (the exact-fallback retry changes them for one call)
    DeviceBuffer nodes, wnodes, tris, spheres, bxdfs, objects, instances, instEntry, textures, textured, images, texels, ewaLut, envTables, alphas, alphaTex, triAlpha, triAttr, triS, uv, materials, lights, distTable, perms, permSums, primes, media, triMediumIn, triMediumOut, sobolMatrices, vdcSobol, vdcSobolInv, noisePerm;
    // work buffers (sized on first render, reused)
    int capacity = 0;
    DeviceBuffer sceneCopy;  // DScene::self
    DeviceBuffer tsOverflow;  // tsBatched: the flag a draw beyond the sample arrays raises
    DeviceBuffer bxdfsPk, matPk;     // the constant BxDF lists as PkLobe records + where each material's starts (k_shade<3>)
    DeviceBuffer matLobes, matHead;  // k_material: the BxDF lists and shading frames of the hits on materials with textured parameters (MatPre)
    int matStride = 0;               // the largest such list of this scene, 0: materials are evaluated inside the shading kernel
    DeviceBuffer shadeOrder, primClass, volPre;  // k_shade_order: the order buffer of the main queue, the primitives' material classes, volpath's pre-drawn medium samples
    bool volOrder = false;  // volpath launches shade medium vertices and surface vertices in separate waves (scenes with homogeneous media only)
    DeviceBuffer animXf;  // scenes with moving instances: the interpolated matrices per closest-hit result
    DeviceBuffer qo[4], qd[4], counts, hitsMain, hitInst, occluded, stL, stBeta, stMeta, pdLight, pdMis, pdBeta, pdInfo, traceCn,
        lightTests, filmDev, straysDev, nStraysDev, cullGuard, cursors, cursors2;
    hipStream_t shadowStream = nullptr;  // any-hit launches run here, concurrently with the next closest-hit launch
    hipEvent_t evShaded = nullptr, evShadowed = nullptr;
    bool cullTripped = false;  // the last call raised k_trace's cull guard (checkCullGuard)
    bool overlapShadow = false;  // PG_OVERLAP_SHADOW=1: any-hit launch on a second stream beside the closest-hit launch (per-kernel times then overlap)
    // PathIntegrator frames of scenes without BSSRDF materials: a vertex's direct lighting is added by the shading launch of the path's next vertex
    // (QueueState::pend) and k_resolve runs over the listed vertices only.  PG_RESOLVE=pass: the full-queue k_resolve launch per bounce instead
    bool resolveFused = true;
    DeviceBuffer qsPend[2], pendList;  // QueueState::pend of the two main queues; PendJoin::list
    // test-path buffers
    DeviceBuffer tO, tD, tCount, tHit, tT, tOcc;  // the test queue; a closest-hit launch's records and t, an any-hit launch's answers
    DeviceBuffer stageIn, stageOut;  // the queries' host arrays staged, one arena per direction (Staging)
    DeviceBuffer tInst, tXf;  // pg_intersect_at's instances and interpolated matrices of the hits (queryScene)
    DeviceBuffer mqO, mqD, mqCount, mqState, mqIsect;  // the medium queries: the second queue of the walk, its state by ray, a pass's interactions by entry
    DeviceBuffer ssO[3], ssD[3], ssCount, ssState, ssXf;  // the subsurface queries: the job queue and the two probe queues, the SssState by ray with chain_rays, the chosen hits' matrices
    DeviceBuffer cqFrame;  // the camera queries and a scattering query's differentials: the call's LensFrame (PG_LENS_FRAME_BYTES)
    LensFrame cqHead = {};  // ... and what the call uploads into it (kept here: the copy is asynchronous)
    PgCounters counters;
    std::vector<hipEvent_t> events;
    bool hasNullMaterial = false;
    bool maySpecularLobes = false;  // pgh_scene_may_add_specular_lobes of the description (pg_render_direct's checks)
    DeviceBuffer directAcc;  // pg_render_direct: two float4 per path slot, the accumulators Ld (one light's samples) and Lall (the lights' sum) of pg_direct.h
    // VolPathIntegrator work buffers (sized on the first volpath render)
    int volCapacity = 0;
    int nMedia = 0;
    DeviceBuffer vqo[2], vqd[2], vCounts, volMedium, trAcc[2], volP1[3], misLi, pdLi, hitT;
    DeviceBuffer qsL[2], qsBeta[2], qsMeta[2], qsMedium[2];  // path state in queue order (qsMedium: volpath)
    DeviceBuffer bssrdfs, materialBssrdf, bssrdfTables;  // subsurface scattering (ABI 24)
    DeviceBuffer grids, mediaGrid, gridDensity, gridVertex;  // GridDensityMedium (ABI 23); the two-phase shading's per-slot vertex record
    // the BSSRDF branch of Li: per-slot state between entry and exit vertex (SssState), the job queue, two probe queues
    DeviceBuffer sssPo, sssFrame[3], sssCoef[2], sssTarget, sssCount, sssHit, sssHitO, sssHitD, sssHitInst, sssHitXf, sssMedium, sssQo[3], sssQd[3], sssCounts, sssTail;
    int sssCapacity = 0;
    DeviceBuffer lightHot;  // DScene::lightHot
    DeviceBuffer haltonDims;  // DScene::haltonDims
    DeviceBuffer lensFrame;  // realistic-camera frames: the per-slot sample weights (+ differentials in textured scenes); absent otherwise
    DeviceBuffer cmaxmin, tsState, ts1, ts2;  // tile-serial samplers: CMaxMinDist, the tiles' sampler states and sample arrays
    DeviceBuffer voxelSlot, voxelRequests, voxelCounters, retryList;  // sparse "spatial" light tables (DScene::sparseLights)
    int poolSlots = 0, poolUsed = 0, nVoxelsTotal = 0;
    DeviceBuffer shardFilm, gatherDev;  // pg_render_sharded: this device's packed shard [film | strays | count]; on rank 0's device the gathered frame
    int qsCapacity = 0;
};

extern "C" {

const char *pg_last_error(void) { return g_lastError.c_str(); }

int pg_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return setError(PG_ERR_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}
int pg_set_device(int device) {
    HIP_TRY(hipSetDevice(device));
    return PG_OK;
}

void pg_scene_destroy(PgScene *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    for (hipEvent_t e : s->events) (void)hipEventDestroy(e);
    if (s->evShaded) (void)hipEventDestroy(s->evShaded);
    if (s->evShadowed) (void)hipEventDestroy(s->evShadowed);
    if (s->shadowStream) (void)hipStreamDestroy(s->shadowStream);
    delete s;
}

// alloc + copy; for 0 bytes nothing is copied and the buffer's pointer stays null
static hipError_t upload(DeviceBuffer &b, const void *src, size_t bytes) {
    hipError_t e = b.alloc(bytes);
    if (e == hipSuccess && bytes) e = hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice);
    return e;
}

// The description is checked and laid out on the host (pg_prepare_scene, pg_scene_prep.h) before anything is allocated: a refused
// scene never reaches the device, and from here on only the device can fail.
int pg_scene_create(const PgSceneDesc *desc, PgScene **out) {
    if (!desc || !out) return setError(PG_ERR_INVALID, "pg_scene_create: null argument");
    *out = nullptr;
    if (!pgAbiAccepted(desc->abi_version)) return setError(PG_ERR_INVALID, "ABI version %d, expected %d", desc->abi_version, PG_ABI_VERSION);  // (PgSceneDesc is the same in 29 and 30)
    // (P may be absent when no primitive is a triangle -- a scene of quadrics only: every triangle's indices are checked against n_verts)
    if (desc->n_tris < 0 || desc->n_nodes < 0 || desc->n_verts < 0 || (desc->n_tris > 0 && (!desc->nodes || !desc->indices || (desc->n_verts > 0 && !desc->P))))
        return setError(PG_ERR_INVALID, "pg_scene_create: malformed geometry arrays");
    if (desc->n_grids < 0 || (desc->n_grids > 0 && (!desc->grids || !desc->media_grid || !desc->grid_density)))
        return setError(PG_ERR_INVALID, "pg_scene_create: malformed grid-medium tables");
    if (desc->n_bssrdfs < 0 || (desc->n_bssrdfs > 0 && (!desc->bssrdfs || !desc->material_bssrdf || !desc->bssrdf_tables)))
        return setError(PG_ERR_INVALID, "pg_scene_create: malformed BSSRDF tables");
    int ndev = 0, device = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return setError(PG_ERR_DEVICE, "no HIP device visible (there is no CPU fallback)");
    HIP_TRY(hipGetDevice(&device));
    const TraceConfig trace = default_trace_config();
    PreparedScene ps;
    std::string err;
    const int status = pg_prepare_scene(desc, trace.depth, ps, err);
    if (status != PG_OK) return setError(status, "%s", err.c_str());
    PgScene *s = new PgScene;
    s->callerAbi = desc->abi_version;
    s->device = device;
    s->trace = trace;
    memset(&s->counters, 0, sizeof(s->counters));
    s->matStride = ps.matStride; s->volOrder = ps.volOrder; s->hasNullMaterial = ps.hasNullMaterial; s->nMedia = ps.nMedia;
    s->nVoxelsTotal = ps.nVoxelsTotal; s->poolSlots = ps.poolSlots;
    s->maySpecularLobes = pgh_scene_may_add_specular_lobes(desc) != 0;
    DScene &d = s->d;
    d = ps.d;
#define FAIL(code, ...) do { int c_ = setError(code, __VA_ARGS__); pg_scene_destroy(s); return c_; } while (0)
#define HIP_TRY_S(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) FAIL(PG_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); } while (0)
    // --- one upload per buffer: the description's own arrays (spans), then the arrays the preparation built
#define UP_SPAN(x) HIP_TRY_S(upload(s->x, ps.x.p, ps.x.bytes))
#define UP_VEC(x) HIP_TRY_S(upload(s->x, ps.x.data(), ps.x.size() * sizeof(ps.x[0])))
    UP_SPAN(nodes); UP_SPAN(instances); UP_SPAN(spheres); UP_SPAN(bxdfs); UP_SPAN(lights); UP_SPAN(envTables);
    UP_SPAN(textures); UP_SPAN(textured); UP_SPAN(images); UP_SPAN(texels); UP_SPAN(ewaLut); UP_SPAN(noisePerm);
    UP_SPAN(alphas); UP_SPAN(triAlpha); UP_SPAN(media); UP_SPAN(triMediumIn); UP_SPAN(triMediumOut);
    UP_SPAN(bssrdfs); UP_SPAN(materialBssrdf); UP_SPAN(bssrdfTables); UP_SPAN(grids); UP_SPAN(mediaGrid); UP_SPAN(gridDensity);
    UP_SPAN(perms); UP_SPAN(permSums); UP_SPAN(cmaxmin); UP_SPAN(sobolMatrices); UP_SPAN(vdcSobol); UP_SPAN(vdcSobolInv);
    UP_VEC(wnodes); UP_VEC(objects); UP_VEC(instEntry); UP_VEC(tris); UP_VEC(uv); UP_VEC(triAttr); UP_VEC(triS);
    UP_VEC(materials); UP_VEC(bxdfsPk); UP_VEC(matPk); UP_VEC(primClass); UP_VEC(lightHot); UP_VEC(distTable);
    UP_VEC(primes); UP_VEC(haltonDims); UP_VEC(alphaTex);
#undef UP_SPAN
#undef UP_VEC
    // --- the "spatial" light distribution (the uniform / power table was uploaded above): a dense table, filled below, or the sparse pool
    if (ps.denseVoxels) HIP_TRY_S(s->distTable.alloc(ps.denseVoxels * ps.distStride * sizeof(float)));
    if (d.sparseLights) {
        const size_t total = (size_t)s->nVoxelsTotal;
        HIP_TRY_S(s->distTable.alloc((size_t)s->poolSlots * ps.distStride * sizeof(float)));
        HIP_TRY_S(s->voxelSlot.alloc(total * sizeof(int)));
        HIP_TRY_S(hipMemset(s->voxelSlot.p, 0xff, total * sizeof(int)));  // -1: not requested
        HIP_TRY_S(s->voxelRequests.alloc(total * sizeof(int)));
        HIP_TRY_S(s->voxelCounters.alloc(2 * sizeof(int)));
        HIP_TRY_S(hipMemset(s->voxelCounters.p, 0, 2 * sizeof(int)));
    }
    // --- every pointer of the device's scene
    d.nodes = (const float4 *)s->nodes.p; d.wnodes = (const float4 *)s->wnodes.p; d.tris = (const float4 *)s->tris.p;
    d.triAttr = (const float4 *)s->triAttr.p; d.triS = (const float4 *)s->triS.p; d.alphaUV = (const float *)s->uv.p;
    d.spheres = (const PgSphere *)s->spheres.p; d.objects = (const DObject *)s->objects.p;
    d.instances = (const PgInstance *)s->instances.p; d.instEntry = (const DInstEntry *)s->instEntry.p;
    d.materials = (const PgMaterial *)s->materials.p; d.bxdfs = (const PgBxDF *)s->bxdfs.p;
    d.bxdfsPk = (const float4 *)s->bxdfsPk.p; d.matPk = (const int2 *)s->matPk.p; d.primClass = (const unsigned char *)s->primClass.p;
    d.lights = (const PgLight *)s->lights.p; d.lightHot = (const float4 *)s->lightHot.p; d.envTables = (const float *)s->envTables.p;
    d.textures = (const PgTexture *)s->textures.p; d.textured = (const PgTexturedMaterial *)s->textured.p; d.noisePerm = (const int *)s->noisePerm.p;
    d.images = (const PgImage *)s->images.p; d.texels = (const float *)s->texels.p; d.ewaLut = (const float *)s->ewaLut.p;
    d.alphas = (const PgAlphaMask *)s->alphas.p; d.triAlpha = (const int *)s->triAlpha.p; d.alphaTex = (const DAlphaTex *)s->alphaTex.p;
    d.bssrdfs = (const PgBSSRDF *)s->bssrdfs.p; d.materialBssrdf = (const int *)s->materialBssrdf.p; d.bssrdfTables = (const float *)s->bssrdfTables.p;
    d.media = (const PgMedium *)s->media.p; d.triMediumIn = (const int *)s->triMediumIn.p; d.triMediumOut = (const int *)s->triMediumOut.p;
    d.grids = (const PgDensityGrid *)s->grids.p; d.mediaGrid = (const int *)s->mediaGrid.p; d.gridDensity = (const float *)s->gridDensity.p;
    d.perms = (const uint16_t *)s->perms.p; d.permSums = (const int32_t *)s->permSums.p; d.primes = (const int32_t *)s->primes.p;
    d.haltonDims = (const int4 *)s->haltonDims.p; d.cmaxmin = (const uint32_t *)s->cmaxmin.p;
    d.sobolMatrices = (const uint32_t *)s->sobolMatrices.p; d.vdcSobol = (const uint64_t *)s->vdcSobol.p; d.vdcSobolInv = (const uint64_t *)s->vdcSobolInv.p;
    d.distTable = (const float *)s->distTable.p;
    d.voxelSlot = (int *)s->voxelSlot.p; d.voxelRequests = (int *)s->voxelRequests.p; d.voxelCounters = (int *)s->voxelCounters.p;
    if (ps.denseVoxels) {  // every voxel up front: they are pure functions of the voxel
        launch_light_tables(d, (float *)s->distTable.p, (int)ps.denseVoxels, 0);
        HIP_TRY_S(hipGetLastError());
        HIP_TRY_S(hipDeviceSynchronize());
    }
    HIP_TRY_S(s->traceCn.alloc(sizeof(TraceCounters) * 3));  // closest hit, any hit, and launches that are not the reference's (second walk of a BSSRDF probe chain)
    HIP_TRY_S(hipMemset(s->traceCn.p, 0, s->traceCn.bytes));
    HIP_TRY_S(s->cursors.alloc(2 * PG_REGIONS * PG_COUNT_STRIDE * sizeof(int)));
    HIP_TRY_S(s->cursors2.alloc(2 * PG_REGIONS * PG_COUNT_STRIDE * sizeof(int)));
    HIP_TRY_S(hipStreamCreateWithFlags(&s->shadowStream, hipStreamNonBlocking));
    HIP_TRY_S(hipEventCreateWithFlags(&s->evShaded, hipEventDisableTiming));
    HIP_TRY_S(hipEventCreateWithFlags(&s->evShadowed, hipEventDisableTiming));
    if (const char *e = getenv("PG_OVERLAP_SHADOW")) s->overlapShadow = atoi(e) != 0;
    if (const char *e = getenv("PG_RESOLVE")) s->resolveFused = strcmp(e, "pass") != 0;
    HIP_TRY_S(s->cullGuard.alloc(sizeof(int) * 2 + 8 * sizeof(unsigned long long)));  // the guard word (+ the counters of the PG_TRACE_STATS experiment build)
    HIP_TRY_S(hipMemset(s->cullGuard.p, 0, s->cullGuard.bytes));
    HIP_TRY_S(s->lightTests.alloc(sizeof(unsigned long long) * PG_LIGHT_TEST_SHARDS * PG_LIGHT_TEST_STRIDE));
    HIP_TRY_S(hipMemset(s->lightTests.p, 0, s->lightTests.bytes));
    HIP_TRY_S(s->sceneCopy.alloc(sizeof(DScene)));
    d.self = (const DScene *)s->sceneCopy.p;
    HIP_TRY_S(hipMemcpy(s->sceneCopy.p, &d, sizeof(DScene), hipMemcpyHostToDevice));
    *out = s;
    return PG_OK;
#undef FAIL
#undef HIP_TRY_S
}

// k_trace's early-cull margin is exact while no ray accepts more than TR_MAX_ACCEPTED hits (pg_traverse.hip); otherwise
// the kernel raises this flag and the call fails instead of returning a possibly different image.
// (g: the guard word as read back)
static int cullGuardStatus(PgScene *s, int g) {
    if (g) {
        HIP_TRY(hipMemset(s->cullGuard.p, 0, sizeof(int)));
        s->cullTripped = true;  // the entry points then repeat the call without the margin (exact by construction, slower)
        return setError(PG_ERR_OVERFLOW, "a ray accepted more than 4096 successive hits: the far-child cull margin is no longer provably exact");
    }
    return PG_OK;
}
static int checkCullGuard(PgScene *s) {
    int g = 0;
    HIP_TRY(hipMemcpy(&g, s->cullGuard.p, sizeof(int), hipMemcpyDeviceToHost));
    return cullGuardStatus(s, g);
}
// Runs `call`; if a ray outran the early-cull margin's proof (sorted stacks of alpha cards can do that), runs it again with the
// margin disabled -- every far child then waits on the stack for the reference's own test at pop time -- with the counters put
// back to where they were, so the result and its statistics are those of one exact pass.
static int withExactFallback(PgScene *s, const std::function<int()> &call) {
    const PgCounters saved = s->counters;
    TraceCounters savedDev[2];
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpy(savedDev, s->traceCn.p, sizeof(savedDev), hipMemcpyDeviceToHost));
    std::vector<unsigned long long> savedLt(PG_LIGHT_TEST_SHARDS * PG_LIGHT_TEST_STRIDE);
    HIP_TRY(hipMemcpy(savedLt.data(), s->lightTests.p, s->lightTests.bytes, hipMemcpyDeviceToHost));
    s->cullTripped = false;
    int st = call();
    if (st != PG_ERR_OVERFLOW || !s->cullTripped) return st;
    s->counters = saved;
    HIP_TRY(hipMemcpy(s->traceCn.p, savedDev, sizeof(savedDev), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->lightTests.p, savedLt.data(), s->lightTests.bytes, hipMemcpyHostToDevice));
    const TraceConfig cfg = s->trace;  // per scene: another host thread's scene (pg_render_sharded) keeps its own margin
    s->trace.cullK = 3e38f;
    s->trace.maxAccepted = 0x7fffffff;  // nothing to guard: no far child is culled early any more
    s->cullTripped = false;
    st = call();
    s->trace = cfg;
    return st;
}

int pg_render_tile_count(const PgRenderDesc *desc) {
    if (!desc) return setError(PG_ERR_INVALID, "pg_render_tile_count: null argument");
    PgRenderDesc current;
    return pgTileCount(pgCurrentRenderDesc(desc, current));
}

// Queue geometry for a batch of `capacity` path slots: PG_REGIONS regions of regionCap entries (multiple of 256) such
// that the blocks of one XCD (b % 8) can never overflow their region.
// `slack`: twice the room (sparse light tables: entries re-shaded in a second pass append from other blocks than their own)
static int regionCapFor(int capacity, bool slack = false) {
    int nblk = (capacity + 255) / 256;
    return ((nblk + PG_REGIONS - 1) / PG_REGIONS) * 256 * (slack ? 2 : 1);
}
// Entries of one queue -- and of every per-entry work buffer -- for a frame of `capacity` path slots (>= capacity); asked once per frame
static size_t queueEntries(const PgScene *s, int capacity) { return (size_t)regionCapFor(capacity, s->d.sparseLights != 0) * PG_REGIONS; }
static const int QSTRIDE = PG_REGIONS * PG_COUNT_STRIDE;  // ints of counter storage per queue

// The four groups of work buffers: each grows when its capacity field says so (n = queueEntries(s, capacity)); the last three fill the kernels' view
static int ensureWorkBuffers(PgScene *s, int capacity, size_t n) {
    if (s->capacity >= capacity) return PG_OK;
    if (s->d.sparseLights) HIP_TRY(s->retryList.alloc(n * sizeof(int)));
    // (scenes with moving instances: one float per entry behind `d`, the rays' times: PG_QUEUE_TIMES)
    for (int i = 0; i < 4; ++i) { HIP_TRY(s->qo[i].alloc(n * sizeof(float4))); HIP_TRY(s->qd[i].alloc(n * (sizeof(float4) + (s->d.hasMotion ? sizeof(float) : 0)))); }
    HIP_TRY(s->counts.alloc(5 * PG_REGIONS * PG_COUNT_STRIDE * sizeof(int)));  // the four queues' counters, then PendJoin::listCounts
    // (grid media: a third part -- the transmittance rays must leave the main rays' hits alone for the second shading phase)
    const size_t hitParts = s->d.nGrids > 0 ? 3 : 2;
    HIP_TRY(s->hitsMain.alloc(hitParts * n * sizeof(float4)));
    if (s->d.primClass || s->volOrder) HIP_TRY(s->shadeOrder.alloc(n * sizeof(int)));
    if (s->volOrder) HIP_TRY(s->volPre.alloc(n * sizeof(float2)));
    if (s->matStride > 0) {  // k_material's lists and frames, one set per main-queue entry; no room: the shading kernel evaluates materials itself
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) { freeB = 0; (void)hipGetLastError(); }
        const size_t recBytes = 3 * sizeof(float4);  // one packed BxDF record
        const size_t want = n * ((size_t)s->matStride * recBytes + 2 * sizeof(float4)), have = s->matLobes.bytes + s->matHead.bytes;
        s->matLobes.release(); s->matHead.release();
        // (everything else of this function and the integrator's own state -- about 600 B per slot -- is still to be allocated)
        // (a list's record index r * plane + p is a 32-bit product in the kernels: plane * stride must stay below 2^31)
        const bool fits = want + n * 700 + ((size_t)1 << 30) <= freeB + have && n * (size_t)s->matStride < ((size_t)1 << 31);
        if (!fits || s->matLobes.alloc(n * (size_t)s->matStride * recBytes) != hipSuccess || s->matHead.alloc(n * 2 * sizeof(float4)) != hipSuccess) {
            s->matLobes.release(); s->matHead.release(); (void)hipGetLastError();
        }
    }
    if (s->d.nInstances > 0) { HIP_TRY(s->hitInst.alloc(hitParts * n * sizeof(int))); s->d.hitInst = (int *)s->hitInst.p; }
    if (s->d.hasMotion) {  // InterpolatedPrimToWorld per closest-hit result on a moving instance (pg_motion.h)
        HIP_TRY(s->animXf.alloc((s->d.hasNest ? 2 : 1) * hitParts * n * PG_XF_STRIDE * sizeof(float)));  // (hasNest: a second half for the inner transform)
        s->d.animXf = (float *)s->animXf.p;
        s->d.nestXfOff = (int)(hitParts * n);
    }  // main-queue hits, then MIS-queue hits at offset n (one launch fills both)
    HIP_TRY(s->occluded.alloc(n * sizeof(int)));
    HIP_TRY(s->stL.alloc(PG_LENS_FRAME_BYTES + n * sizeof(float4)));  /* (a realistic frame's LensFrame in front of the array) */ HIP_TRY(s->stBeta.alloc(n * sizeof(float4))); HIP_TRY(s->stMeta.alloc(n * sizeof(int4)));
    HIP_TRY(s->pdLight.alloc(n * sizeof(float4))); HIP_TRY(s->pdMis.alloc(n * sizeof(float4))); HIP_TRY(s->pdBeta.alloc(n * sizeof(float4))); HIP_TRY(s->pdInfo.alloc(n * sizeof(int4)));
    s->capacity = capacity;
    return PG_OK;
}
// VolPathIntegrator: the per-slot medium state, and in vq the second halves of the through-ray ping-pong (the first halves are q[2] and q[3])
static int ensureVolBuffers(PgScene *s, int capacity, size_t n, VolState &vs, RayQueue vq[2]) {
    if (s->volCapacity < capacity) {
        for (int i = 0; i < 2; ++i) { HIP_TRY(s->vqo[i].alloc(n * sizeof(float4))); HIP_TRY(s->vqd[i].alloc(n * (sizeof(float4) + (s->d.hasMotion ? sizeof(float) : 0)))); HIP_TRY(s->trAcc[i].alloc(n * sizeof(float4))); }
        for (int i = 0; i < 3; ++i) HIP_TRY(s->volP1[i].alloc(n * sizeof(float4)));
        HIP_TRY(s->vCounts.alloc(2 * QSTRIDE * sizeof(int)));
        HIP_TRY(s->volMedium.alloc(n * sizeof(int)));
        HIP_TRY(s->misLi.alloc(n * sizeof(float4)));
        HIP_TRY(s->pdLi.alloc(n * sizeof(float4)));
        HIP_TRY(s->hitT.alloc((s->d.nGrids > 0 ? 3 : 2) * n * sizeof(float)));
        s->volCapacity = capacity;
    }
    if (s->d.nGrids > 0 && s->gridVertex.bytes < n * sizeof(float4)) HIP_TRY(s->gridVertex.alloc(n * sizeof(float4)));
    vs.medium = (int *)s->volMedium.p;
    for (int i = 0; i < 2; ++i) vs.trAcc[i] = (float4 *)s->trAcc[i].p;
    for (int i = 0; i < 3; ++i) vs.p1[i] = (float4 *)s->volP1[i].p;
    vs.misLi = (float4 *)s->misLi.p; vs.pdLi = (float4 *)s->pdLi.p;
    for (int i = 0; i < 2; ++i) { vq[i].o = (float4 *)s->vqo[i].p; vq[i].d = (float4 *)s->vqd[i].p; vq[i].counts = (int *)s->vCounts.p + i * QSTRIDE; }
    return PG_OK;
}
// PathIntegrator, and VolPathIntegrator on scenes without BSSRDF materials or grid media (whose probe-chain / two-phase kernels find a
// path's state by its slot): L / beta / meta (/ the ray's medium) in queue order beside each main queue.  (The kernels are compiled for one
// or the other: k_shade's QSTATE.)
static int ensureQueueState(PgScene *s, int capacity, size_t n, bool vol, bool direct, PathState &ps) {
    const bool volQ = vol && s->d.nBssrdfs == 0 && s->d.nGrids == 0;
    if (vol && !volQ) return PG_OK;
    if (s->qsCapacity < capacity) {
        for (int i = 0; i < 2; ++i) { HIP_TRY(s->qsL[i].alloc(n * sizeof(float4))); HIP_TRY(s->qsBeta[i].alloc(n * sizeof(float4))); HIP_TRY(s->qsMeta[i].alloc(n * sizeof(int4))); }
        s->qsCapacity = capacity;
    }
    if (volQ && s->qsMedium[0].bytes < n * sizeof(int)) for (int i = 0; i < 2; ++i) HIP_TRY(s->qsMedium[i].alloc(n * sizeof(int)));
    const bool pendQ = !vol && !direct && s->resolveFused && s->d.nBssrdfs == 0;  // (bouncesPath's frames)
    if (pendQ && s->pendList.bytes < n * sizeof(int)) {
        for (int i = 0; i < 2; ++i) HIP_TRY(s->qsPend[i].alloc(n * sizeof(float4)));
        HIP_TRY(s->pendList.alloc(n * sizeof(int)));
    }
    for (int i = 0; i < 2; ++i) { ps.qs[i].L = (float4 *)s->qsL[i].p; ps.qs[i].beta = (float4 *)s->qsBeta[i].p; ps.qs[i].meta = (int4 *)s->qsMeta[i].p;
                                  ps.qs[i].medium = volQ ? (int *)s->qsMedium[i].p : nullptr; ps.qs[i].pend = pendQ ? (float4 *)s->qsPend[i].p : nullptr; }
    return PG_OK;
}
// Subsurface scattering: per-slot state of the BSSRDF branch with its job queue, and in sssP the two probe queues
static int ensureSssBuffers(PgScene *s, int capacity, size_t n, SssState &sq, RayQueue sssP[2]) {
    if (s->sssCapacity < capacity) {
        HIP_TRY(s->sssPo.alloc(n * sizeof(float4))); HIP_TRY(s->sssTarget.alloc(n * sizeof(float4))); HIP_TRY(s->sssCount.alloc(n * sizeof(int2)));
        for (int i = 0; i < 3; ++i) HIP_TRY(s->sssFrame[i].alloc(n * sizeof(float4)));
        for (int i = 0; i < 2; ++i) HIP_TRY(s->sssCoef[i].alloc(n * sizeof(float4)));
        HIP_TRY(s->sssHit.alloc(n * sizeof(float4))); HIP_TRY(s->sssHitO.alloc(n * sizeof(float4))); HIP_TRY(s->sssHitD.alloc(n * sizeof(float4)));
        HIP_TRY(s->sssHitInst.alloc(n * sizeof(int)));
        if (s->d.hasMotion) HIP_TRY(s->sssHitXf.alloc((s->d.hasNest ? 2 : 1) * n * PG_XF_STRIDE * sizeof(float)));  // the chosen hit's interpolated instance matrices
        HIP_TRY(s->sssMedium.alloc(n * sizeof(int2)));
        for (int i = 0; i < 3; ++i) { HIP_TRY(s->sssQo[i].alloc(n * sizeof(float4))); HIP_TRY(s->sssQd[i].alloc(n * (sizeof(float4) + (s->d.hasMotion ? sizeof(float) : 0)))); }  // (+ the probe rays' times: PG_QUEUE_TIMES)
        HIP_TRY(s->sssCounts.alloc(3 * QSTRIDE * sizeof(int)));
        HIP_TRY(s->sssTail.alloc(QSTRIDE * sizeof(int)));
        s->sssCapacity = capacity;
    }
    sq.po = (float4 *)s->sssPo.p; sq.target = (float4 *)s->sssTarget.p; sq.count = (int2 *)s->sssCount.p;
    for (int i = 0; i < 3; ++i) sq.frame[i] = (float4 *)s->sssFrame[i].p;
    for (int i = 0; i < 2; ++i) sq.coef[i] = (float4 *)s->sssCoef[i].p;
    sq.hit = (float4 *)s->sssHit.p; sq.hitO = (float4 *)s->sssHitO.p; sq.hitD = (float4 *)s->sssHitD.p; sq.hitInst = (int *)s->sssHitInst.p; sq.hitXf = (float *)s->sssHitXf.p; sq.hitXfNest = (int)n; sq.medium = (int2 *)s->sssMedium.p;
    sq.qjob.o = (float4 *)s->sssQo[0].p; sq.qjob.d = (float4 *)s->sssQd[0].p; sq.qjob.counts = (int *)s->sssCounts.p;
    for (int i = 0; i < 2; ++i) { sssP[i].o = (float4 *)s->sssQo[1 + i].p; sssP[i].d = (float4 *)s->sssQd[1 + i].p; sssP[i].counts = (int *)s->sssCounts.p + (1 + i) * QSTRIDE; }
    return PG_OK;
}

static hipEvent_t getEvent(PgScene *s, size_t idx) {
    while (s->events.size() <= idx) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        s->events.push_back(e);
    }
    return s->events[idx];
}

extern "C++" {  // (templates)
// HIP events around one launch on `st` (the stream the kernel runs on); per-kernel times are only meaningful while the
// any-hit launch does not share the chip with the closest-hit launch (PG_OVERLAP_SHADOW=0, the default).  `on` = false: no event is
// touched (the tile-serial mode: its hundreds of thousands of small launches would each need a pair of events).
struct LaunchTimer {
    PgScene *s = nullptr;
    bool on = false; size_t ev = 2;  // (events 0 and 1 are the frame's)
    std::vector<std::pair<size_t, int>> timed;  // (event index, kernel: 0 closest-hit, 1 any-hit, 2 shade, 3 resolve, 4 generate, 5 film)
    template <class F> int run(int kind, hipStream_t st, F &&launch) {
        if (!on) { launch(); return PG_OK; }
        hipEvent_t a = getEvent(s, ev), b = getEvent(s, ev + 1);
        if (!a || !b) return setError(PG_ERR_DEVICE, "hipEventCreate failed");
        timed.push_back({ev, kind}); ev += 2;
        HIP_TRY(hipEventRecord(a, st)); launch(); HIP_TRY(hipEventRecord(b, st));
        return PG_OK;
    }
};
// What the bounce loops and the frame drivers share
struct FrameCtx {
    PgScene *s = nullptr; const PgRenderDesc *rd = nullptr; hipStream_t stream = nullptr;
    RenderParams rp = {};
    DScene d;  // the frame's scene: s->d with this frame's sampler state (ts*); s->d itself is never written by a render
    bool vol = false, tileSerial = false, sssOn = false;
    size_t nQueue = 0;  // queueEntries of the frame's capacity
    PathState ps = {}; VolState vs = {}; SssState sq = {};
    RayQueue q[4] = {}, vq[2] = {}, sssP[2] = {};  // main ping-pong, shadow (2), MIS (3); the through rays' second halves; the probe queues
    int *counts = nullptr, *cursors = nullptr, *cullGuard = nullptr;
    float4 *hits = nullptr, *hitsMis = nullptr;
    TraceCounters *cnClosest = nullptr, *cnShadow = nullptr;
    unsigned long long *lightTests = nullptr;
    PgFilmPixel *dFilm = nullptr; PgStraySample *dStrays = nullptr; int *dNStrays = nullptr, maxStrays = 0;  // device film / stray buffers (the caller's when mem == DEVICE)
    BounceLimits lim = {};
    const PgDirectLightingDesc *direct = nullptr;  // a DirectLightingIntegrator frame (pg_render_direct): stepsDirect instead of the bounce loops
    float4 *directLd = nullptr, *directAll = nullptr;  // its per-slot accumulators (PgScene::directAcc)
    DeviceBuffer countLog;  // per-bounce queue sizes, copied back after the batch for the ray statistics
    std::vector<int> hostCounts, curQueueOfBounce, blk, vblk;  // (blk / vblk: host copies of the counter blocks of q[] / vq[])
    uint64_t closestRays = 0, shadowRays = 0, cameraRays = 0, closestLaunches = 0, shadowLaunches = 0;
    uint64_t shadeLaunches = 0, resolveLaunches = 0, shadeItems = 0, misRays = 0, shadingModes = 0;
    LaunchTimer timer;
};

// sum of a queue's region counters in a host copy of the counter block
static uint64_t queueTotal(const int *blk, int qi) { uint64_t t = 0; for (int r = 0; r < PG_REGIONS; ++r) t += (uint64_t)blk[qi * QSTRIDE + r * PG_COUNT_STRIDE]; return t; }
// the counter blocks of the four queues (volpath: and of vq[]) back into c.blk (c.vblk)
static int readCounts(FrameCtx &c) {
    HIP_TRY(hipMemcpyAsync(c.blk.data(), c.counts, 4 * QSTRIDE * sizeof(int), hipMemcpyDeviceToHost, c.stream));
    if (c.vol) HIP_TRY(hipMemcpyAsync(c.vblk.data(), c.s->vCounts.p, 2 * QSTRIDE * sizeof(int), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return PG_OK;
}
// one queue's counters on the device -> its size (one wait)
static int queueSize(hipStream_t stream, const int *deviceCounts, uint64_t &total) {
    int blk[QSTRIDE];
    HIP_TRY(hipMemcpyAsync(blk, deviceCounts, sizeof(blk), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    total = queueTotal(blk, 0);
    return PG_OK;
}
// PgCounters::shading_modes: which k_shade<MODE> this frame's shading launches are (pg_shade_mode, the launch functions' own choice)
static void noteShading(FrameCtx &c, const DScene &dsc, bool vol, bool sss, bool gridPhase) {
    const int mode = pg_shade_mode(dsc, c.rp, vol, sss, gridPhase);
    c.shadingModes |= 1ull << mode;
    if (mode == 3) c.shadingModes |= PG_SHADING_MATERIAL_PREPASS;
    if (mode == 2 && !gridPhase && !(sss && dsc.nBssrdfs > 0) && c.s->matStride > 0) c.shadingModes |= PG_SHADING_LISTS_DID_NOT_FIT;
}
// Sparse "spatial" light tables: after a shading launch, compute the distributions of the voxels its lanes asked for and
// shade the entries that waited for them (one host round trip per launch while the table warms up; none once every
// voxel the image touches exists -- the tables stay with the scene).
template <class F> static int settleLightTables(FrameCtx &c, F &&reshade) {
    PgScene *s = c.s;
    if (!c.d.sparseLights) return PG_OK;
    int cnt[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(cnt, s->voxelCounters.p, sizeof(cnt), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    if (cnt[0] == 0 && cnt[1] == 0) return PG_OK;
    if (s->poolUsed + cnt[0] > s->poolSlots)
        return setError(PG_ERR_UNSUPPORTED, "spatial light distribution: %d voxels x %d lights exceed the table pool (%d voxels); use "
                                            "\"lightsamplestrategy\" \"power\" or \"uniform\"", s->poolUsed + cnt[0], c.d.nLights, s->poolSlots);
    launch_light_tables_sparse(c.d, (float *)s->distTable.p, (const int *)s->voxelRequests.p, cnt[0], s->poolUsed, c.stream);
    s->poolUsed += cnt[0];
    HIP_TRY(hipMemsetAsync(s->voxelCounters.p, 0, sizeof(cnt), c.stream));
    if (cnt[1] > 0) { c.rp.retryCount = cnt[1]; reshade(); c.rp.retryCount = 0; }
    return PG_OK;
}
// The start of a batch of c.rp.capacity path slots: the queues' geometry, empty queues, the camera rays into the first main queue
static int startBatch(FrameCtx &c, const std::function<void()> &generate) {
    const int cap = regionCapFor(c.rp.capacity, c.d.sparseLights != 0);
    for (int i = 0; i < 4; ++i) c.q[i].regionCap = cap;
    c.vq[0].regionCap = c.vq[1].regionCap = c.sq.qjob.regionCap = c.sssP[0].regionCap = c.sssP[1].regionCap = cap;
    c.curQueueOfBounce.clear();
    HIP_TRY(hipMemsetAsync(c.counts, 0, 4 * QSTRIDE * sizeof(int), c.stream));
    return c.timer.run(4, c.stream, generate);
}
// The probe chains of SeparableBSSRDF::Sample_Sp for the nJobs entries of the job queue sq.qjob, walked twice through the traversal kernel over the
// two probe queues: pass 1 counts the hits on the material, pass 2 stops at the chosen one.  One counter read-back per step.  `d` says where the
// probe rays' instances go, `hits` where their hits go; vol: the volpath variant of k_sss_probe.  The first walk's launches count into cn and the
// caller accounts for each of its steps in firstWalkStep(queue, rays), between the step's two launches; the second walk repeats queries the reference
// makes once: its traversal work goes to cn + 2 and its rays are not counted.  `entry`: the entry point that runs, for the error text
template <class F> static int sssProbeChains(const char *entry, PgScene *s, const DScene &d, const SssState &sq, const RayQueue probe[2], float4 *hits, TraceCounters *cn,
                                             uint64_t nJobs, bool vol, hipStream_t stream, F &&firstWalkStep) {
    for (int pass = 1; pass <= 2; ++pass) {
        RayQueue curQ = sq.qjob;
        uint64_t nRays = nJobs;
        for (int step = 0; nRays > 0; ++step) {
            if (step > 1000000) return setError(PG_ERR_DEVICE, "%s: a BSSRDF probe chain did not terminate", entry);
            RayQueue outQ = probe[step & 1];
            HIP_TRY(hipMemsetAsync(outQ.counts, 0, QSTRIDE * sizeof(int), stream));
            launch_closest(d, s->trace, curQ, hits, nullptr, pass == 1 ? cn : cn + 2, (int *)s->cursors.p, (int *)s->cullGuard.p, stream);
            if (pass == 1) firstWalkStep(curQ, nRays);
            launch_sss_probe(d, sq, pass, curQ, hits, outQ, stream, vol, vol && step == 0);
            if (int e = queueSize(stream, outQ.counts, nRays)) return e;
            curQ = outQ;
        }
    }
    return PG_OK;
}
// ... for the paths k_shade handed over (c.sq.qjob)
static int sssProbeChains(FrameCtx &c, const DScene &d, float4 *hits, uint64_t nJobs, bool vol) {
    return sssProbeChains("pg_render", c.s, d, c.sq, c.sssP, hits, c.cnClosest, nJobs, vol, c.stream,
                          [&c](const RayQueue &, uint64_t nRays) { c.closestRays += nRays; ++c.closestLaunches; });
}

// volpath's through rays: kind 0 = light samples (q[2] <-> vq[0]), kind 1 = BSDF / phase samples (q[3] <-> vq[1]), re-traced
// until none is left under way
static int throughRays(FrameCtx &c, const DScene &dv, float *hitT) {
    const hipStream_t stream = c.stream; const int n1 = (int)c.nQueue;
    if (c.d.nGrids > 0) {
        // ratio tracking draws from the path's sampler: a path's kind-0 ray (visibility.Tr) runs to its end before
        // its kind-1 ray (IntersectTr after the BSDF sample) starts, as in EstimateDirect; one queue pair at a time
        for (int kind = 0; kind < 2; ++kind) {
            RayQueue tk[2] = {kind == 0 ? c.q[2] : c.q[3], c.vq[kind]};
            int tc = 0;
            for (int pass = 0;; ++pass) {
                if (pass > 100000) return setError(PG_ERR_DEVICE, "pg_render: transmittance loop did not terminate");
                if (int e = readCounts(c)) return e;
                const uint64_t nk = tc == 0 ? queueTotal(c.blk.data(), 2 + kind) : queueTotal(c.vblk.data(), kind);
                if (nk == 0) break;
                // (results at the offset the kind's through kernel reads them from)
                const size_t off = (size_t)(1 + kind) * n1;  // part 0 keeps the main rays' hits for phase 2
                DScene dk = dv;
                if (dk.hitInst) dk.hitInst += off;
                if (dk.animXf) dk.animXf += off * PG_XF_STRIDE;
                if (int e = c.timer.run(0, stream, [&] { launch_closest(dk, c.s->trace, tk[tc], c.hits + off, hitT + off, c.cnClosest, c.cursors, c.cullGuard, stream); })) return e;
                ++c.closestLaunches; c.closestRays += nk;
                HIP_TRY(hipMemsetAsync(tk[tc ^ 1].counts, 0, QSTRIDE * sizeof(int), stream));
                launch_through(dv, c.ps, c.vs, kind, tk[tc], c.hits, hitT, (int)off, tk[tc ^ 1], stream, &c.rp);
                tc ^= 1;
            }
        }
        return PG_OK;
    }
    RayQueue tq[2][2] = {{c.q[2], c.vq[0]}, {c.q[3], c.vq[1]}};
    int tcur = 0;
    for (int pass = 0;; ++pass) {
        if (pass > 100000) return setError(PG_ERR_DEVICE, "pg_render: transmittance loop did not terminate");
        if (int e = readCounts(c)) return e;
        const uint64_t n0 = tcur == 0 ? queueTotal(c.blk.data(), 2) : queueTotal(c.vblk.data(), 0);
        const uint64_t n1q = tcur == 0 ? queueTotal(c.blk.data(), 3) : queueTotal(c.vblk.data(), 1);
        if (n0 + n1q == 0) break;
        if (int e = c.timer.run(0, stream, [&] { launch_closest2(dv, c.s->trace, tq[0][tcur], tq[1][tcur], c.hits, n1, c.cnClosest, c.cursors, c.cullGuard, stream, hitT); })) return e;
        ++c.closestLaunches; c.closestRays += n0 + n1q;
        HIP_TRY(hipMemsetAsync(tq[0][tcur ^ 1].counts, 0, QSTRIDE * sizeof(int), stream));
        HIP_TRY(hipMemsetAsync(tq[1][tcur ^ 1].counts, 0, QSTRIDE * sizeof(int), stream));
        launch_through(dv, c.ps, c.vs, 0, tq[0][tcur], c.hits, hitT, 0, tq[0][tcur ^ 1], stream);
        launch_through(dv, c.ps, c.vs, 1, tq[1][tcur], c.hits, hitT, n1, tq[1][tcur ^ 1], stream);
        tcur ^= 1;
    }
    return PG_OK;
}

// One batch of paths from their camera rays (`generate` fills the first main queue) to their film samples (`film`): all the
// bounces of the c.rp.capacity path slots described by c.rp, under VolPathIntegrator::Li (volpath.cpp:72-186).  Per loop iteration:
// closest-hit(main rays, with the hits' ray parameters) -> shade with medium sampling -> the transmittance rays of the light samples
// and of the BSDF/phase samples, re-traced until none is left under way (light.cpp:63-81, scene.cpp:57-70) -> resolve.
// Crossing a surface without a material does not count as a bounce, so the loop runs until the queue is empty.
static int bouncesVolpath(FrameCtx &c, const std::function<void()> &generate, const std::function<void()> &film) {
    PgScene *s = c.s; const hipStream_t stream = c.stream; RayQueue *const q = c.q;
    if (int e = startBatch(c, generate)) return e;
    int cur = 0;  // main queue index (0/1 ping-pong); 2 = light-sample rays, 3 = BSDF / phase-sample rays
    DScene dv = c.d;
    dv.ext = 1;  // the general shading kernels
    float *hitT = (float *)s->hitT.p;
    launch_fill_int(c.vs.medium, c.rd->camera_medium + 1, c.rp.capacity, stream);  // camera rays start in the camera's medium (camera.h:78)
    if (int e = readCounts(c)) return e;
    uint64_t nMain = queueTotal(c.blk.data(), cur);
    c.cameraRays += nMain;
    const SssState *sssArg = c.sssOn ? &c.sq : nullptr;
    // a scene with a grid medium shades in two phases around the transmittance rays (k_shade<., ., ., GRID>)
    const bool gridOn = c.d.nGrids > 0;
    float4 *gridVertex = (float4 *)s->gridVertex.p;
    // (GlobalSamplers, dense light tables: the tile-serial streams and the deferred vertices of sparse tables draw in the shading kernel)
    float2 *volPre = (s->volOrder && !c.tileSerial && !c.d.sparseLights) ? (float2 *)s->volPre.p : nullptr;
    for (int iter = 0; nMain > 0; ++iter) {
        if (iter > 100000) return setError(PG_ERR_DEVICE, "pg_render: volpath loop did not terminate");
        const int nxt = cur ^ 1;
        if (int e = c.timer.run(0, stream, [&] { launch_closest(dv, s->trace, q[cur], c.hits, hitT, c.cnClosest, c.cursors, c.cullGuard, stream); })) return e;
        ++c.closestLaunches; c.closestRays += nMain; c.shadeItems += nMain;
        HIP_TRY(hipMemsetAsync(c.counts + nxt * QSTRIDE, 0, QSTRIDE * sizeof(int), stream));
        HIP_TRY(hipMemsetAsync(c.counts + 2 * QSTRIDE, 0, 2 * QSTRIDE * sizeof(int), stream));
        if (c.sssOn) HIP_TRY(hipMemsetAsync(c.sq.qjob.counts, 0, QSTRIDE * sizeof(int), stream));
        c.rp.volPre = volPre;
        c.rp.order = (c.d.primClass || volPre) ? (const int *)s->shadeOrder.p : nullptr;  // (the second phase of a grid scene takes the same order)
        auto shade = [&](int phase) { launch_shade_vol(dv, c.rp, c.ps, c.vs, q[cur], c.hits, hitT, q[nxt], q[2], q[3], c.lightTests, stream, sssArg, gridVertex, phase, phase == 2 ? 0 : cur); };
        if (int e = c.timer.run(2, stream, [&] { launch_shade_order_vol(dv, c.rp, c.ps, c.vs, q[cur], c.hits, hitT, (int *)s->shadeOrder.p, volPre, stream, cur); shade(gridOn ? 1 : 0); })) return e;
        ++c.shadeLaunches; noteShading(c, dv, true, sssArg != nullptr, gridOn);
        if (int e = settleLightTables(c, [&] { shade(gridOn ? 1 : 0); })) return e;
        if (int e = throughRays(c, dv, hitT)) return e;
        if (int e = c.timer.run(3, stream, [&] { launch_resolve_vol(dv, c.ps, c.vs, q[cur], stream, cur); })) return e;
        ++c.resolveLaunches;
        if (gridOn) {  // phase 2: the vertices' next directions, drawn behind the transmittance rays' numbers
            if (int e = c.timer.run(2, stream, [&] { shade(2); })) return e;
            ++c.shadeLaunches;
            if (int e = readCounts(c)) return e;
        }
        if (c.sssOn) {
            // ---- the BSSRDF branch (volpath.cpp:151-176) of the paths k_shade handed over: probe chains (two walks), exit
            // vertices, their transmittance rays and resolve; the exit vertices' next rays join q[nxt], which is
            // traced as a whole at the start of the next iteration
            uint64_t nJobs = 0;
            if (int e = queueSize(c.stream, c.sq.qjob.counts, nJobs)) return e;
            if (nJobs > 0) {
                if (int e = sssProbeChains(c, dv, c.hits, nJobs, true)) return e;
                HIP_TRY(hipMemsetAsync(c.counts + 2 * QSTRIDE, 0, 2 * QSTRIDE * sizeof(int), stream));
                // (a grid medium's ratio tracking draws from the paths' samplers: the exit vertices' transmittance rays run between their direct
                // lighting and their next directions, as at k_shade's vertices -- k_sss_exit in two phases; gridVertex is free again by now)
                launch_sss_exit(dv, c.rp, c.ps, c.sq, q[nxt], q[2], q[3], c.lightTests, stream, nxt, true, c.vs, gridOn ? 1 : 0, gridVertex);
                ++c.shadeLaunches; c.shadeItems += nJobs;
                if (int e = throughRays(c, dv, hitT)) return e;
                launch_resolve_vol(dv, c.ps, c.vs, c.sq.qjob, stream);
                ++c.resolveLaunches;
                if (gridOn) { launch_sss_exit(dv, c.rp, c.ps, c.sq, q[nxt], q[2], q[3], c.lightTests, stream, nxt, true, c.vs, 2, gridVertex); ++c.shadeLaunches; }
            }
            if (int e = readCounts(c)) return e;
        }
        // the last pass of the through loop read the counters: the main queue's size comes from the same block
        nMain = queueTotal(c.blk.data(), nxt);
        cur = nxt;
    }
    film();  // (not timed: volpath's film launch never was)
    HIP_TRY(hipStreamSynchronize(stream));
    return PG_OK;
}

// The same under PathIntegrator::Li.  Launch order per bounce b (one stream): shade(b) -> any-hit(shadow rays of b) -> closest-hit(main
// rays of b+1 and MIS rays of b in ONE launch) -> resolve(b).  The first closest-hit launch traces the camera rays alone.
static int bouncesPath(FrameCtx &c, const std::function<void()> &generate, const std::function<void()> &film) {
    PgScene *s = c.s; const PgRenderDesc *rd = c.rd;
    const hipStream_t stream = c.stream; RayQueue *const q = c.q;
    if (int e = startBatch(c, generate)) return e;
    int cur = 0;  // main queue index (0/1 ping-pong); 2 = shadow, 3 = MIS
    if (int e = c.timer.run(0, stream, [&] { launch_closest(c.d, s->trace, q[cur], c.hits, nullptr, c.cnClosest, c.cursors, c.cullGuard, stream); })) return e;
    ++c.closestLaunches;
    const SssState *sssArg = c.sssOn ? &c.sq : nullptr;
    // (no QueueState::pend: PG_RESOLVE=pass, or BSSRDF materials, whose exit vertices k_sss_exit shades: k_resolve over the whole queue)
    PendJoin pj = {(const int *)s->occluded.p, nullptr, nullptr, false};
    if (c.ps.qs[0].pend && !c.sssOn) { pj.listCounts = c.counts + 4 * QSTRIDE; pj.list = (int *)s->pendList.p; }
    int iters = 0;
    for (int bounce = 0; bounce < c.lim.maxIters; ++bounce, ++iters) {
        const int nxt = cur ^ 1;
        HIP_TRY(hipMemsetAsync(c.counts + nxt * QSTRIDE, 0, QSTRIDE * sizeof(int), stream));
        HIP_TRY(hipMemsetAsync(c.counts + 2 * QSTRIDE, 0, (pj.list ? 3 : 2) * QSTRIDE * sizeof(int), stream));  // (and the list of this bounce's launch)
        if (c.sssOn) HIP_TRY(hipMemsetAsync(c.sq.qjob.counts, 0, QSTRIDE * sizeof(int), stream));
        c.rp.order = c.d.primClass ? (const int *)s->shadeOrder.p : nullptr;
        pj.first = bounce == 0;
        auto shade = [&] { launch_shade(c.d, c.rp, c.ps, q[cur], c.hits, q[nxt], q[2], q[3], c.lightTests, stream, cur, sssArg, pj); };
        if (int e = c.timer.run(2, stream, [&] { launch_shade_order(c.d, q[cur], c.hits, (int *)s->shadeOrder.p, stream); shade(); })) return e;
        ++c.shadeLaunches; noteShading(c, c.d, false, sssArg != nullptr, false);
        if (int e = settleLightTables(c, shade)) return e;
        // paths that reach maxdepth neither continue nor sample lights (path.cpp:104): nothing left to trace
        const bool lastDepth = !s->hasNullMaterial && bounce >= rd->max_depth;
        if (!lastDepth) {
            // The shadow rays of this bounce and the closest-hit rays of the next depend only on shade(b): the any-hit
            // launch goes to a second stream so that its blocks fill the chip while the closest-hit launch's
            // persistent waves drain (and vice versa); resolve(b) joins both.
            // (tile-serial samplers: a handful of rays per launch, each a chain of dependent fetches -- both launches are
            // latency-bound and run side by side)
            // (overlapShadow: the environment's PG_OVERLAP_SHADOW at pg_scene_create, then pg_scene_set_option -- a caller such as bench.py times
            // frames with the overlap and takes per-kernel times from a serialised frame of the same scene)
            const bool overlap = s->overlapShadow || c.tileSerial;
            hipStream_t sst = overlap ? s->shadowStream : stream;
            if (overlap) { HIP_TRY(hipEventRecord(s->evShaded, stream)); HIP_TRY(hipStreamWaitEvent(sst, s->evShaded, 0)); }
            if (int e = c.timer.run(1, sst, [&] { launch_anyhit(c.d, s->trace, q[2], (int *)s->occluded.p, c.cnShadow, (int *)s->cursors2.p, sst); })) return e;
            ++c.shadowLaunches;
            if (overlap) HIP_TRY(hipEventRecord(s->evShadowed, sst));
            if (int e = c.timer.run(0, stream, [&] { launch_closest2(c.d, s->trace, q[nxt], q[3], c.hits, (int)c.nQueue, c.cnClosest, c.cursors, c.cullGuard, stream); })) return e;
            ++c.closestLaunches;
            if (overlap) HIP_TRY(hipStreamWaitEvent(stream, s->evShadowed, 0));
            if (int e = c.timer.run(3, stream, [&] {
                    if (pj.list) launch_resolve_list(c.d, c.ps, q[cur], q[3], pj, c.hitsMis, stream, cur, c.lightTests);
                    else launch_resolve(c.d, c.ps, q[cur], q[3], (const int *)s->occluded.p, c.hitsMis, stream, cur, c.lightTests);
                })) return e;
            ++c.resolveLaunches;
        }
        // log this bounce's queue sizes
        HIP_TRY(hipMemcpyAsync((int *)c.countLog.p + 4 * QSTRIDE * (size_t)bounce, c.counts, 4 * QSTRIDE * sizeof(int), hipMemcpyDeviceToDevice, stream));
        c.curQueueOfBounce.push_back(cur);
        if (c.sssOn && !lastDepth) {
            // ---- the BSSRDF branch of Li (path.cpp:152-174) for the paths k_shade handed over: the probe chains, then the exit
            // vertices: their shadow / MIS rays, the tail of the next bounce's queue that their next rays form, and the resolve of
            // their direct lighting.
            uint64_t nJobs = 0;
            if (int e = queueSize(c.stream, c.sq.qjob.counts, nJobs)) return e;
            if (nJobs > 0) {
                const size_t n1 = (size_t)q[0].regionCap * PG_REGIONS;
                DScene dprobe = c.d;  // the probe rays' hits go where the MIS rays' went (k_resolve is done with those)
                if (dprobe.hitInst) dprobe.hitInst += n1;
                if (dprobe.animXf) dprobe.animXf += n1 * PG_XF_STRIDE;
                if (int e = sssProbeChains(c, dprobe, c.hitsMis, nJobs, false)) return e;
                HIP_TRY(hipMemcpyAsync(s->sssTail.p, c.counts + nxt * QSTRIDE, QSTRIDE * sizeof(int), hipMemcpyDeviceToDevice, stream));
                HIP_TRY(hipMemsetAsync(c.counts + 2 * QSTRIDE, 0, 2 * QSTRIDE * sizeof(int), stream));
                launch_sss_exit(c.d, c.rp, c.ps, c.sq, q[nxt], q[2], q[3], c.lightTests, stream, nxt, false, c.vs);
                ++c.shadeLaunches; c.shadeItems += nJobs;
                launch_anyhit(c.d, s->trace, q[2], (int *)s->occluded.p, c.cnShadow, (int *)s->cursors2.p, stream);
                ++c.shadowLaunches;
                launch_closest2(c.d, s->trace, q[nxt], q[3], c.hits, (int)n1, c.cnClosest, c.cursors, c.cullGuard, stream, nullptr, (const int *)s->sssTail.p);
                ++c.closestLaunches;
                launch_resolve(c.d, c.ps, c.sq.qjob, q[3], (const int *)s->occluded.p, c.hitsMis, stream, cur);
                ++c.resolveLaunches;
                uint64_t nSh = 0, nMis = 0;
                if (int e = queueSize(c.stream, c.counts + 2 * QSTRIDE, nSh)) return e;
                if (int e = queueSize(c.stream, c.counts + 3 * QSTRIDE, nMis)) return e;
                c.shadowRays += nSh; c.closestRays += nMis; c.misRays += nMis;  // (the next rays are counted with the next bounce's queue)
            }
        }
        cur = nxt;
        if ((s->hasNullMaterial && bounce >= rd->max_depth) || (bounce >= PG_MAX_BLIND_BOUNCES && bounce % 32 == 0)) {
            if (int e = readCounts(c)) return e;
            if (queueTotal(c.blk.data(), cur) == 0) { ++iters; break; }
        }
    }
    if (iters == c.lim.maxIters && c.lim.wantIters > c.lim.maxIters) {  // the last allowed bounce: is anything still alive?
        if (int e = readCounts(c)) return e;
        if (queueTotal(c.blk.data(), cur) != 0) return setError(PG_ERR_UNSUPPORTED, "paths longer than %lld vertices (maxdepth %d)", PG_MAX_BOUNCES, rd->max_depth);
    }
    if (int e = c.timer.run(5, stream, film)) return e;
    c.hostCounts.resize(4 * QSTRIDE * (size_t)iters);  // read back once per batch (pinned copy not needed: tiny)
    HIP_TRY(hipMemcpyAsync(c.hostCounts.data(), c.countLog.p, sizeof(int) * 4 * QSTRIDE * (size_t)iters, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int b = 0; b < iters; ++b) {
        const int *blk = c.hostCounts.data() + 4 * QSTRIDE * (size_t)b;
        const uint64_t nMain = queueTotal(blk, c.curQueueOfBounce[b]), nShadow = queueTotal(blk, 2), nMis = queueTotal(blk, 3);
        c.closestRays += nMain + nMis; c.shadowRays += nShadow; c.shadeItems += nMain; c.misRays += nMis;
        if (getenv("PG_PRINT_COUNTS"))
            fprintf(stderr, "pg_render: bounce %d main %llu shadow %llu mis %llu\n", b, (unsigned long long)nMain, (unsigned long long)nShadow, (unsigned long long)nMis);
    }
    if (iters > 0) c.cameraRays += queueTotal(c.hostCounts.data(), c.curQueueOfBounce[0]);
    return PG_OK;
}
// The same under DirectLightingIntegrator::Li without its specular bounces (directlighting.cpp:62-95; pg_direct.h).  A "level" is one main queue: the camera
// rays' hits, then -- scenes with surfaces that have no material -- the hits of the rays re-spawned behind such surfaces, until none is left.  Launch order per
// level (one stream): for every (light, sample) step direct(step) -> any-hit(its shadow rays) -> closest-hit(its BSDF-sampled rays) -> resolve(step) into the
// slots' Ld; after a light's last sample fold(Ld / nSamples -> Lall); after the last light fold(Lall -> L); then closest-hit(the re-spawned rays).
static int stepsDirect(FrameCtx &c, const std::function<void()> &generate, const std::function<void()> &film) {
    PgScene *s = c.s; const PgRenderDesc *rd = c.rd; const PgDirectLightingDesc *dl = c.direct;
    const hipStream_t stream = c.stream; RayQueue *const q = c.q;
    // the steps of one level and the divisions that follow them
    struct Step { DirectStep ds; float foldLd; bool foldAll; };  // foldLd != 0: after this step Lall += Ld / foldLd (strategy 1: L += Ld / foldLd); foldAll: then L += Lall
    std::vector<Step> steps;
    const int nLights = dl->n_lights;
    if (nLights == 0) steps.push_back({{1, -1, 0, 0, 0}, 0.f, false});  // directlighting.cpp:82: no light sampling at all
    else if (dl->strategy == 1) steps.push_back({{1, -2, 6, 0, 0}, 1.f / (float)nLights, false});  // Get1D at dimension 5, then uLight, uScattering
    else
        for (int j = 0; j < nLights; ++j) {
            // max_depth 0: no array was requested (directlighting.cpp:53): one Get2D pair per light from the sequential dimensions and no division
            const int n = rd->max_depth >= 1 ? dl->light_samples[j] : 1;
            for (int k = 0; k < n; ++k)
                steps.push_back({{steps.empty() ? 1 : 0, j, 5 + 4 * j, rd->max_depth >= 1 ? n : 0, k}, k == n - 1 ? (float)n : 0.f, k == n - 1 && j == nLights - 1});
        }
    const size_t nSteps = steps.size();
    if (c.countLog.bytes < sizeof(int) * 4 * QSTRIDE * nSteps) HIP_TRY(c.countLog.alloc(sizeof(int) * 4 * QSTRIDE * nSteps));
    HIP_TRY(hipMemsetAsync(c.directLd, 0, 2 * sizeof(float4) * (size_t)(c.directAll - c.directLd), stream));
    if (int e = startBatch(c, generate)) return e;
    int cur = 0;
    if (int e = c.timer.run(0, stream, [&] { launch_closest(c.d, s->trace, q[cur], c.hits, nullptr, c.cnClosest, c.cursors, c.cullGuard, stream); })) return e;
    ++c.closestLaunches;
    DScene dmis = c.d;  // the BSDF-sampled rays' hits, instances and interpolated matrices go behind the main queue's, which every step of a level reads again
    if (dmis.hitInst) dmis.hitInst += c.nQueue;
    if (dmis.animXf) dmis.animXf += c.nQueue * PG_XF_STRIDE;
    PathState acc = c.ps;  // k_resolve adds a step's EstimateDirect to "the path's L by slot": the Ld accumulator
    acc.L = c.directLd;
    c.hostCounts.resize(4 * QSTRIDE * nSteps);
    for (long long level = 0;; ++level) {
        if (level >= c.lim.maxIters) return setError(PG_ERR_UNSUPPORTED, "camera rays through more than %lld surfaces without a material", (long long)c.lim.maxIters);
        const int nxt = cur ^ 1;
        HIP_TRY(hipMemsetAsync(c.counts + nxt * QSTRIDE, 0, QSTRIDE * sizeof(int), stream));
        for (size_t si = 0; si < nSteps; ++si) {
            const Step &st = steps[si];
            HIP_TRY(hipMemsetAsync(c.counts + 2 * QSTRIDE, 0, 2 * QSTRIDE * sizeof(int), stream));
            if (int e = c.timer.run(2, stream, [&] { launch_direct(c.d, c.rp, c.ps, q[cur], c.hits, q[nxt], q[2], q[3], c.lightTests, st.ds, stream); })) return e;
            ++c.shadeLaunches;
            if (st.ds.light != -1) {
                if (int e = c.timer.run(1, stream, [&] { launch_anyhit(c.d, s->trace, q[2], (int *)s->occluded.p, c.cnShadow, (int *)s->cursors2.p, stream); })) return e;
                ++c.shadowLaunches;
                if (int e = c.timer.run(0, stream, [&] { launch_closest(dmis, s->trace, q[3], c.hitsMis, nullptr, c.cnClosest, c.cursors, c.cullGuard, stream); })) return e;
                ++c.closestLaunches;
                if (int e = c.timer.run(3, stream, [&] {
                        launch_resolve(c.d, acc, q[cur], q[3], (const int *)s->occluded.p, c.hitsMis, stream, 0, nullptr);
                        if (st.foldLd != 0.f) launch_direct_fold(c.directLd, dl->strategy == 1 ? c.ps.L : c.directAll, st.foldLd, c.rp.capacity, stream);
                        if (st.foldAll) launch_direct_fold(c.directAll, c.ps.L, 1.f, c.rp.capacity, stream);
                    })) return e;
                ++c.resolveLaunches;
            }
            HIP_TRY(hipMemcpyAsync((int *)c.countLog.p + 4 * QSTRIDE * si, c.counts, 4 * QSTRIDE * sizeof(int), hipMemcpyDeviceToDevice, stream));
        }
        // this level's queue sizes: the rays the reference's statistics count, and whether a ray was re-spawned
        HIP_TRY(hipMemcpyAsync(c.hostCounts.data(), c.countLog.p, sizeof(int) * 4 * QSTRIDE * nSteps, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        const uint64_t nMain = queueTotal(c.hostCounts.data(), cur), nNext = queueTotal(c.hostCounts.data(), nxt);
        c.closestRays += nMain; c.shadeItems += nMain * nSteps;
        if (level == 0) c.cameraRays += nMain;
        for (size_t si = 0; si < nSteps; ++si) {
            if (steps[si].ds.light == -1) continue;
            const int *blk = c.hostCounts.data() + 4 * QSTRIDE * si;
            const uint64_t nShadow = queueTotal(blk, 2), nMis = queueTotal(blk, 3);
            c.shadowRays += nShadow; c.closestRays += nMis; c.misRays += nMis;
        }
        if (nNext == 0) break;
        if (int e = c.timer.run(0, stream, [&] { launch_closest(c.d, s->trace, q[nxt], c.hits, nullptr, c.cnClosest, c.cursors, c.cullGuard, stream); })) return e;
        ++c.closestLaunches;
        cur = nxt;
    }
    return c.timer.run(5, stream, film);
}
static int tracePaths(FrameCtx &c, const std::function<void()> &generate, const std::function<void()> &film) { if (c.direct) return stepsDirect(c, generate, film); return c.vol ? bouncesVolpath(c, generate, film) : bouncesPath(c, generate, film); }

// The PixelSamplers (stratified, 02sequence, maxmindist) fall back to their tile's RNG stream only for draws beyond their
// "dimensions" (sampler.cpp:108-134).  PathIntegrator::Li draws at most 1 + 2 maxdepth one-dimensional numbers (time; light choice and
// roulette per vertex) and 2 + 3 maxdepth two-dimensional ones (film, lens; uLight, uScattering, the next direction per vertex):
// with that many sampled dimensions StartPixel alone consumes the stream, every pixel's arrays can be generated ahead, and the
// paths run as one wavefront like the GlobalSamplers' (tsBatched).  Not for volpath (a ray through material-less surfaces samples
// its medium an unbounded number of times), materials with a BSSRDF, or sparse light tables (their deferred vertices re-draw).
// The arrays of all local tiles are one allocation: taken here, before any state is set, so that a device without the room
// (less memory free, a large scene beside them) renders tile by tile as before instead of failing with PG_ERR_DEVICE.
static bool reserveSampleArrays(PgScene *s, const PgRenderDesc *rd) {
    if (!(rd->sampler > PG_SAMPLER_RANDOM && rd->integrator == 0 && s->d.nBssrdfs == 0 && !s->d.sparseLights && rd->sampler_dims <= 63 &&
          rd->sampler_dims >= 2 + 3 * (long long)rd->max_depth && !(getenv("PG_TS_BATCHED") && atoi(getenv("PG_TS_BATCHED")) == 0))) return false;
    const size_t nArr = (size_t)pgTileCount(rd) * 256 * (size_t)rd->sampler_dims * (size_t)rd->spp;
    size_t freeB = 0, totalB = 0;
    if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) { freeB = 0; (void)hipGetLastError(); }
    const size_t have = s->ts1.bytes + s->ts2.bytes;  // (buffers of an earlier frame are given back first)
    if (!(nArr * 12 <= ((size_t)48 << 30) && nArr * 12 + ((size_t)2 << 30) <= freeB + have)) return false;
    s->ts1.release(); s->ts2.release();
    const bool ok = s->ts1.alloc(sizeof(float) * (nArr + 1)) == hipSuccess && s->ts2.alloc(sizeof(float) * 2 * (nArr + 1)) == hipSuccess;
    if (!ok) { s->ts1.release(); s->ts2.release(); (void)hipGetLastError(); }
    return ok;
}

// The frame's work buffers for `capacity` path slots and the views of them the kernels take
static int setUpFrame(FrameCtx &c, int capacity) {
    PgScene *s = c.s;
    c.nQueue = queueEntries(s, capacity);
    if (int e = ensureWorkBuffers(s, capacity, c.nQueue)) return e;
    if (c.vol) if (int e = ensureVolBuffers(s, capacity, c.nQueue, c.vs, c.vq)) return e;
    if (int e = ensureQueueState(s, capacity, c.nQueue, c.vol, c.direct != nullptr, c.ps)) return e;
    c.sssOn = s->d.nBssrdfs > 0;
    if (c.sssOn) if (int e = ensureSssBuffers(s, capacity, c.nQueue, c.sq, c.sssP)) return e;
    c.d = s->d;
    c.hits = (float4 *)s->hitsMain.p; c.hitsMis = c.hits + c.nQueue; c.cursors = (int *)s->cursors.p; c.cullGuard = (int *)s->cullGuard.p;
    c.ps.L = (float4 *)((char *)s->stL.p + PG_LENS_FRAME_BYTES); c.ps.beta = (float4 *)s->stBeta.p; c.ps.meta = (int4 *)s->stMeta.p;
    c.ps.pdLight = (float4 *)s->pdLight.p; c.ps.pdMis = (float4 *)s->pdMis.p; c.ps.pdBeta = (float4 *)s->pdBeta.p; c.ps.pdInfo = (int4 *)s->pdInfo.p;
    c.counts = (int *)s->counts.p;
    for (int i = 0; i < 4; ++i) { c.q[i].o = (float4 *)s->qo[i].p; c.q[i].d = (float4 *)s->qd[i].p; c.q[i].counts = c.counts + i * QSTRIDE; }
    c.cnClosest = (TraceCounters *)s->traceCn.p; c.cnShadow = c.cnClosest + 1;
    c.lightTests = (unsigned long long *)s->lightTests.p;
    c.rp.retryList = (int *)s->retryList.p;
    if (s->matLobes.p && s->matHead.p) { c.rp.matPre.lobes = (float4 *)s->matLobes.p; c.rp.matPre.head = (float4 *)s->matHead.p; c.rp.matPre.stride = s->matStride; }
    c.blk.resize(4 * QSTRIDE); c.vblk.resize(2 * QSTRIDE);
    c.lim = pgBounceLimits(c.rd->max_depth, s->hasNullMaterial);
    if (c.direct) {
        if (s->directAcc.bytes < 2 * sizeof(float4) * (size_t)capacity) HIP_TRY(s->directAcc.alloc(2 * sizeof(float4) * (size_t)capacity));
        c.directLd = (float4 *)s->directAcc.p; c.directAll = c.directLd + capacity;
    }
    if (c.rd->camera_type == 3) {  // the realistic camera: the lens block, zeroed statistics and room for the slots' weights, for this frame only
        const bool diffs = s->d.hasTextured != 0;  // (the camera ray's differentials are read at the first textured hit alone)
        const size_t weightBytes = ((size_t)capacity * sizeof(float) + 255) & ~(size_t)255;
        const size_t need = weightBytes + (diffs ? (size_t)capacity * 3 * sizeof(float4) : 0);
        if (s->lensFrame.bytes < need) HIP_TRY(s->lensFrame.alloc(need));
        LensFrame head = {};
        memcpy(&head.lens, &c.rd->n_lens_interfaces, sizeof(PgLensSystem));
        head.weights = (float *)s->lensFrame.p;
        head.differentials = diffs ? (float4 *)((char *)s->lensFrame.p + weightBytes) : nullptr;
        HIP_TRY(hipMemcpy(lens_frame(c.ps.L), &head, sizeof(head), hipMemcpyHostToDevice));
    }
    return PG_OK;
}

// The GlobalSamplers, and the PixelSamplers whose sample arrays were reserved (tsBatched): tile x sample batches, each one wavefront
static int renderBatched(FrameCtx &c, int nLocalTiles, BatchShape shape, bool tsBatched) {
    PgScene *s = c.s; const PgRenderDesc *rd = c.rd; RenderParams &rp = c.rp;
    if (tsBatched) {  // every pixel's sample arrays, one lane per tile (the tile's stream in the reference's pixel order)
        const size_t nArr = (size_t)nLocalTiles * 256 * (size_t)rd->sampler_dims * (size_t)rd->spp;
        HIP_TRY(s->tsState.alloc(sizeof(TileSamplerState) * (size_t)nLocalTiles));
        if (s->ts1.bytes < sizeof(float) * (nArr + 1) || s->ts2.bytes < sizeof(float) * 2 * (nArr + 1)) return setError(PG_ERR_DEVICE, "pg_render: sample arrays not allocated");  // (taken by reserveSampleArrays)
        HIP_TRY(s->tsOverflow.alloc(sizeof(int)));
        HIP_TRY(hipMemsetAsync(s->tsOverflow.p, 0, sizeof(int), c.stream));
        c.d.ts = (TileSamplerState *)s->tsState.p; c.d.ts1 = (float *)s->ts1.p; c.d.ts2 = (float *)s->ts2.p;
        c.d.tsDims = rd->sampler_dims; c.d.tsSpp = rd->spp; c.d.tsBatched = 1; c.d.tsOverflow = (int *)s->tsOverflow.p;
        rp.tileLocal0 = 0; rp.nTilesBatch = nLocalTiles; rp.s0 = 0; rp.sCount = 1; rp.capacity = nLocalTiles;
        launch_ts_init(c.d, rp, c.stream);
        rp.tsGuessSkew = getenv("PG_TS_GUESS_SKEW") ? atoi(getenv("PG_TS_GUESS_SKEW")) : 0;
        launch_ts_start_tile(c.d, rp, c.stream);
    }
    const std::function<void()> generate = [&]() { launch_generate(c.d, rp, c.ps, c.q[0], c.stream); };
    const std::function<void()> film = [&]() { if (rd->filter_general) launch_film_general(rp, c.ps, c.dFilm, c.stream); else launch_film(rp, c.ps, c.dFilm, c.dStrays, c.maxStrays, c.dNStrays, c.stream); };
    for (int tile0 = 0; tile0 < nLocalTiles; tile0 += shape.tiles)
        for (int s0 = 0; s0 < rd->spp; s0 += shape.samples) {
            rp.tileLocal0 = tile0; rp.nTilesBatch = std::min(shape.tiles, nLocalTiles - tile0);
            rp.s0 = s0; rp.sCount = std::min(shape.samples, rd->spp - s0);
            rp.capacity = rp.nTilesBatch * 256 * rp.sCount;
            if (int e = tracePaths(c, generate, film)) return e;
        }
    if (tsBatched) {
        int over = 0;
        HIP_TRY(hipMemcpyAsync(&over, s->tsOverflow.p, sizeof(int), hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        if (over & 2) return setError(PG_ERR_DEVICE, "pg_render: the start offsets of a tile's pixel sample arrays did not converge (k_ts_start_tile, internal error)");
        if (over) return setError(PG_ERR_DEVICE, "pg_render: a path drew beyond the %d sampled dimensions of the batched pixel sampler (internal error)", rd->sampler_dims);
    }
    return PG_OK;
}
// The samplers that draw from one RNG stream per tile (random, stratified, 02sequence, maxmindist): a tile's pixels, a
// pixel's samples and a sample's draws consume the stream in order, and how many numbers a path takes depends on the
// path -- so a tile has ONE path in flight, and the wavefront is one path of every tile: pixel (lx, ly) of all tiles,
// sample by sample (integrator.cpp:247-332).  Tiles clipped by the image skip the pixels they do not have.
static int renderTileSerial(FrameCtx &c, int nLocalTiles) {
    PgScene *s = c.s; const PgRenderDesc *rd = c.rd; RenderParams &rp = c.rp;
    const int nd = rd->sampler == PG_SAMPLER_RANDOM ? 0 : rd->sampler_dims;
    HIP_TRY(s->tsState.alloc(sizeof(TileSamplerState) * (size_t)nLocalTiles));
    HIP_TRY(s->ts1.alloc(sizeof(float) * ((size_t)nLocalTiles * nd * rd->spp + 1)));
    HIP_TRY(s->ts2.alloc(sizeof(float) * 2 * ((size_t)nLocalTiles * nd * rd->spp + 1)));
    c.d.ts = (TileSamplerState *)s->tsState.p; c.d.ts1 = (float *)s->ts1.p; c.d.ts2 = (float *)s->ts2.p;
    c.d.tsDims = nd; c.d.tsSpp = rd->spp;
    rp.tileLocal0 = 0; rp.nTilesBatch = nLocalTiles; rp.s0 = 0; rp.sCount = 1; rp.capacity = nLocalTiles;
    launch_ts_init(c.d, rp, c.stream);
    for (int ly = 0; ly < 16; ++ly)
        for (int lx = 0; lx < 16; ++lx) {
            if (rd->sample_bounds[0] + lx >= rd->sample_bounds[2] || rd->sample_bounds[1] + ly >= rd->sample_bounds[3]) continue;  // no tile has this pixel
            launch_ts_start_pixel(c.d, rp, lx, ly, c.stream);
            for (int sn = 0; sn < rd->spp; ++sn)
                if (int e = tracePaths(c, [&]() { launch_ts_generate(c.d, rp, c.ps, c.q[0], sn, c.stream); },
                                       [&]() { launch_ts_film(c.d, rp, c.ps, c.dFilm, c.dStrays, c.maxStrays, c.dNStrays, c.stream); })) return e;
        }
    return PG_OK;
}

// The film and the stray samples back to the caller (mem == HOST), or the stray count clamped in place; hostNStrays: the samples the frame produced
static int readBackFrame(FrameCtx &c, PgFilmPixel *film, size_t filmBytes, PgStraySample *strays, int32_t *nStrays, int mem, int &hostNStrays) {
    HIP_TRY(hipMemcpyAsync(&hostNStrays, c.dNStrays, sizeof(int), hipMemcpyDeviceToHost, c.stream));
    if (mem == PG_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(film, c.dFilm, filmBytes, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        int nCopy = std::min(hostNStrays, c.maxStrays);
        if (nCopy > 0) HIP_TRY(hipMemcpy(strays, c.dStrays, sizeof(PgStraySample) * (size_t)nCopy, hipMemcpyDeviceToHost));
        *nStrays = nCopy;
    } else {
        HIP_TRY(hipStreamSynchronize(c.stream));
        if (hostNStrays > c.maxStrays) { int v = c.maxStrays; HIP_TRY(hipMemcpy(c.dNStrays, &v, sizeof(int), hipMemcpyHostToDevice)); }
    }
    return PG_OK;
}
// The frame's tallies, the device's traversal and integrator statistics and the event times into the scene's PgCounters
static int accountFrame(FrameCtx &c, hipEvent_t evStart, hipEvent_t evStop) {
    PgScene *s = c.s;
    PgCounters &pc = s->counters;
    TraceCounters tc[2];
    unsigned long long lt = 0;
    HIP_TRY(hipMemcpy(tc, s->traceCn.p, sizeof(tc), hipMemcpyDeviceToHost));
    std::vector<unsigned long long> shards(PG_LIGHT_TEST_SHARDS * PG_LIGHT_TEST_STRIDE);
    HIP_TRY(hipMemcpy(shards.data(), c.lightTests, s->lightTests.bytes, hipMemcpyDeviceToHost));
    for (int i = 0; i < PG_LIGHT_TEST_SHARDS; ++i) lt += shards[(size_t)i * PG_LIGHT_TEST_STRIDE];
    // the integrators' own statistics, words 1 .. 8 of the same shards (pg_kernels.h): like the light tests they run on from pg_counters_reset
    pc.paths_total = pc.paths_zero_radiance = pc.path_length_sum = pc.path_length_count = pc.path_length_min = pc.path_length_max = pc.volume_interactions = pc.surface_interactions = 0;
    unsigned long long minc = 0, maxp = 0;
    for (int i = 0; i < PG_LIGHT_TEST_SHARDS; ++i) {
        const unsigned long long *sh = &shards[(size_t)i * PG_LIGHT_TEST_STRIDE];
        pc.path_length_sum += sh[PG_STAT_LEN_SUM]; pc.path_length_count += sh[PG_STAT_LEN_COUNT];
        minc = std::max(minc, sh[PG_STAT_LEN_MINC]); maxp = std::max(maxp, sh[PG_STAT_LEN_MAXP]);
        pc.paths_total += sh[PG_STAT_PATHS]; pc.paths_zero_radiance += sh[PG_STAT_PATHS_ZERO];
        pc.volume_interactions += sh[PG_STAT_VOLUME]; pc.surface_interactions += sh[PG_STAT_SURFACE];
    }
    if (pc.path_length_count > 0) { pc.path_length_min = 0xffff - minc; pc.path_length_max = maxp - 1; }
    pc.camera_rays += c.cameraRays; pc.closest_rays += c.closestRays; pc.shadow_rays += c.shadowRays;
    if (c.rd->camera_type == 3) {  // the realistic camera's GenerateRay calls; a sample of weight 0 entered no queue but is a camera ray all the same (integrator.cpp:296)
        unsigned long long ls[3];
        HIP_TRY(hipMemcpy(ls, (const char *)lens_frame(c.ps.L) + offsetof(LensFrame, stats), sizeof(ls), hipMemcpyDeviceToHost));
        pc.lens_rays_total += ls[0]; pc.lens_rays_vignetted += ls[1]; pc.camera_rays += ls[2];
    }
    pc.node_visits = tc[0].node_visits + tc[1].node_visits;
    pc.tri_tests = tc[0].tri_tests + tc[1].tri_tests + lt;
    pc.light_tri_tests = lt;
    pc.closest_node_visits = tc[0].node_visits; pc.closest_tri_tests = tc[0].tri_tests;
    pc.shadow_node_visits = tc[1].node_visits; pc.shadow_tri_tests = tc[1].tri_tests;
    pc.closest_launches += c.closestLaunches; pc.shadow_launches += c.shadowLaunches;
    pc.shade_launches += c.shadeLaunches; pc.resolve_launches += c.resolveLaunches; pc.shade_items += c.shadeItems; pc.mis_rays += c.misRays;
    pc.shading_modes |= c.shadingModes;
    for (auto &te : c.timer.timed) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, s->events[te.first], s->events[te.first + 1]) != hipSuccess) continue;
        double *acc[6] = {&pc.closest_ms, &pc.shadow_ms, &pc.shade_ms, &pc.resolve_ms, &pc.generate_ms, &pc.film_ms};
        *acc[te.second] += ms;
    }
    float ms = 0;
    if (hipEventElapsedTime(&ms, evStart, evStop) == hipSuccess) pc.render_ms += ms;
    return PG_OK;
}
}  // extern "C++"

// One frame: check, reserve, set up, drive, read back, account.  The description is checked on the host (pg_check_render_desc,
// pg_render_check.h) before anything is allocated or released.
static int renderFrame(PgScene *s, const PgRenderDesc *rd, PgFilmPixel *film, PgStraySample *strays, int32_t maxStrays, int32_t *nStrays, int mem,
                       void *streamPtr, const PgDirectLightingDesc *dl = nullptr) {
    std::string err;
    RenderSceneFacts facts = {s->nMedia, s->cmaxmin.p != nullptr, s->d.sobolMatrices != nullptr, s->d.perms != nullptr, s->d.nPermDims};
    facts.nLights = s->d.nLights; facts.maySpecularLobes = s->maySpecularLobes;
    if (int st = pg_check_render_desc(rd, facts, err)) return setError(st, "%s", err.c_str());
    if (dl) if (int st = pg_check_direct_desc(rd, dl, facts, err)) return setError(st, "%s", err.c_str());
    // (a DirectLightingIntegrator frame under a PixelSampler draws from its tiles' streams, one camera ray per tile at a time: no arrays ahead)
    const bool tsBatched = !dl && reserveSampleArrays(s, rd);
    HIP_TRY(hipSetDevice(s->device));
    FrameCtx c;
    c.s = s; c.rd = rd; c.stream = (hipStream_t)streamPtr; c.vol = rd->integrator == 1; c.direct = dl;
    c.tileSerial = rd->sampler >= PG_SAMPLER_RANDOM && !tsBatched;
    const int nLocalTiles = pgTileCount(rd);
    c.rp.rd = *rd;
    c.rp.nTilesX = (rd->sample_bounds[2] - rd->sample_bounds[0] + 15) / 16;
    c.rp.nTilesY = (rd->sample_bounds[3] - rd->sample_bounds[1] + 15) / 16;
    // device film / stray buffers (caller's when mem == DEVICE)
    c.dFilm = film; c.dStrays = strays; c.dNStrays = nStrays; c.maxStrays = maxStrays;
    const size_t filmBytes = sizeof(PgFilmPixel) * (size_t)rd->tile_pixels * (size_t)nLocalTiles;
    if (mem == PG_MEM_HOST) {
        HIP_TRY(s->filmDev.alloc(filmBytes));
        HIP_TRY(s->straysDev.alloc(sizeof(PgStraySample) * (size_t)(maxStrays > 0 ? maxStrays : 1)));
        HIP_TRY(s->nStraysDev.alloc(sizeof(int)));
        c.dFilm = (PgFilmPixel *)s->filmDev.p; c.dStrays = (PgStraySample *)s->straysDev.p; c.dNStrays = (int *)s->nStraysDev.p;
    }
    if (filmBytes) HIP_TRY(hipMemsetAsync(c.dFilm, 0, filmBytes, c.stream));
    HIP_TRY(hipMemsetAsync(c.dNStrays, 0, sizeof(int), c.stream));
    if (nLocalTiles == 0) { if (mem == PG_MEM_HOST) *nStrays = 0; return PG_OK; }
    size_t budget = (size_t)1 << 27;
    if (const char *e = getenv("PG_BATCH_PATHS")) { long v = atol(e); if (v >= 256) budget = (size_t)v; }
    const BatchShape shape = pgBatchShape(rd->spp, nLocalTiles, rd->filter_general != 0, budget);
    // tile-serial samplers: one path per tile in flight, slot = the tile's local index
    if (int e = setUpFrame(c, c.tileSerial ? std::max(nLocalTiles, 256) : shape.tiles * 256 * shape.samples)) return e;
    c.timer.s = s; c.timer.on = !c.tileSerial;
    hipEvent_t evStart = getEvent(s, 0), evStop = getEvent(s, 1);
    if (!evStart || !evStop) return setError(PG_ERR_DEVICE, "hipEventCreate failed");
    HIP_TRY(hipEventRecord(evStart, c.stream));
    HIP_TRY(c.countLog.alloc(sizeof(int) * 4 * QSTRIDE * (size_t)(c.lim.maxIters + 1)));
    if (int e = c.tileSerial ? renderTileSerial(c, nLocalTiles) : renderBatched(c, nLocalTiles, shape, tsBatched)) return e;
    HIP_TRY(hipEventRecord(evStop, c.stream));
    HIP_TRY(hipGetLastError());
    int hostNStrays = 0;
    if (int e = readBackFrame(c, film, filmBytes, strays, nStrays, mem, hostNStrays)) return e;
    if (int e = accountFrame(c, evStart, evStop)) return e;
    if (int st2 = checkCullGuard(s)) return st2;
    if (hostNStrays > maxStrays) return setError(PG_ERR_OVERFLOW, "%d stray samples, buffer holds %d", hostNStrays, maxStrays);
    return PG_OK;
}
int pg_render(PgScene *s, const PgRenderDesc *rd, PgFilmPixel *film, PgStraySample *strays, int32_t maxStrays, int32_t *nStrays,
              int mem, void *streamPtr) {
    if (!s || !rd || !film || !nStrays || (maxStrays > 0 && !strays)) return setError(PG_ERR_INVALID, "pg_render: null argument");
    PgRenderDesc current;
    rd = pgCurrentRenderDesc(rd, current);
    return withExactFallback(s, [&]() { return renderFrame(s, rd, film, strays, maxStrays, nStrays, mem, streamPtr); });
}

// DirectLightingIntegrator frames (pg_direct.h): pg_render's frame with the light-sample steps in place of the bounce loops.  Both descriptions are
// checked on the host before anything is allocated (pg_check_render_desc, then pg_check_direct_desc).
int pg_render_direct(PgScene *s, const PgRenderDesc *rd, const PgDirectLightingDesc *dl, PgFilmPixel *film, PgStraySample *strays, int32_t maxStrays,
                     int32_t *nStrays, int mem, void *streamPtr) {
    if (!s || !rd || !dl || !film || !nStrays || (maxStrays > 0 && !strays)) return setError(PG_ERR_INVALID, "pg_render_direct: null argument");
    PgRenderDesc current;
    rd = pgCurrentRenderDesc(rd, current);
    return withExactFallback(s, [&]() { return renderFrame(s, rd, film, strays, maxStrays, nStrays, mem, streamPtr, dl); });
}

// ---- the film gather of pg_render_sharded over RCCL (ncclGather, rccl.h:745) ---------------------------------------
// librccl is opened on the first multi-device render (a single-device process never pays for loading it); one communicator per
// device list, kept for the life of the process.  Every rank sends ONE packed shard [film | strays | count] of the same size (the
// largest shard's: tile counts differ by at most one), the first device receives n of them in rank order.
#ifndef HIP_EMU_H
namespace {
typedef struct ncclComm *PgNcclComm;
struct Rccl {
    int (*CommInitAll)(PgNcclComm *, int, const int *) = nullptr;
    int (*Gather)(const void *, void *, size_t, int, int, PgNcclComm, hipStream_t) = nullptr;  // ncclGather, rccl.h:745
    const char *(*GetErrorString)(int) = nullptr;
    bool ok = false;
    std::string why;
};
Rccl *rcclApi() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) { r.why = std::string("librccl not found: ") + dlerror(); return; }
        r.CommInitAll = (decltype(r.CommInitAll))dlsym(h, "ncclCommInitAll");
        r.Gather = (decltype(r.Gather))dlsym(h, "ncclGather");
        r.GetErrorString = (decltype(r.GetErrorString))dlsym(h, "ncclGetErrorString");
        r.ok = r.CommInitAll && r.Gather && r.GetErrorString;
        if (!r.ok) r.why = "librccl lacks ncclCommInitAll / ncclGather";
    });
    return &r;
}
std::mutex g_commMutex;
std::map<std::vector<int>, std::vector<PgNcclComm>> g_comms;
// communicators of this device list, or null with the reason in `why` (then the caller gathers with peer copies)
const std::vector<PgNcclComm> *shardComms(const std::vector<int> &devices, std::string &why) {
    std::vector<int> sorted = devices;
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) { why = "a device appears twice in the list (RCCL wants one rank per GPU)"; return nullptr; }
    Rccl &r = *rcclApi();
    if (!r.ok) { why = r.why; return nullptr; }
    std::lock_guard<std::mutex> lock(g_commMutex);
    auto it = g_comms.find(devices);
    if (it != g_comms.end()) return &it->second;
    std::vector<PgNcclComm> comms(devices.size(), nullptr);
    const int st = r.CommInitAll(comms.data(), (int)devices.size(), devices.data());
    if (st != 0) { why = std::string("ncclCommInitAll: ") + r.GetErrorString(st); return nullptr; }
    return &(g_comms[devices] = comms);
}
}  // namespace
#endif
// "rccl" / "peer" (+ why RCCL was not used): how the last pg_render_sharded of this process gathered its shards.  The text is
// replaced under a lock and handed out as a pointer that stays valid for the calling thread until its next call.
static std::mutex g_shardTransportMutex;
static std::string g_shardTransport = "none";
const char *pg_shard_transport(void) {
    static thread_local std::string mine;
    std::lock_guard<std::mutex> lock(g_shardTransportMutex);
    mine = g_shardTransport;
    return mine.c_str();
}
int pg_box_filter_needs_gather(const PgRenderDesc *rd) {
    PgRenderDesc current;
    return rd ? pgh_box_filter_needs_gather(pgCurrentRenderDesc(rd, current)) : 0;
}

// ---- one frame over several devices of the node, from one host process ---------------------------------------------------------
// One host thread per device (pg_set_device is per thread); every thread renders its tiles into a packed shard on its own device,
// then ONE ncclGather (RCCL over xGMI) brings the n shards to the first device -- or, where RCCL cannot run (a device that repeats
// in the list, no librccl, PG_SHARD_GATHER=peer), one peer-to-peer copy per rank into the same layout.  No per-bounce
// communication, no reduction: tiles are disjoint.
int pg_render_sharded(PgScene *const *scenes, int32_t n, const PgRenderDesc *desc, PgFilmPixel *const *film, PgStraySample *const *strays,
                      int32_t maxStrays, int32_t *nStrays) {
    if (!scenes || n < 1 || !desc || !film || !nStrays || (maxStrays > 0 && !strays)) return setError(PG_ERR_INVALID, "pg_render_sharded: null argument");
    PgRenderDesc current;
    desc = pgCurrentRenderDesc(desc, current);
    if (desc->tile_first != 0 || desc->tile_step != 1) return setError(PG_ERR_INVALID, "pg_render_sharded: desc must describe the whole frame (tile_first 0, tile_step 1)");
    for (int r = 0; r < n; ++r) if (!scenes[r] || (maxStrays > 0 && !strays[r])) return setError(PG_ERR_INVALID, "pg_render_sharded: null entry for rank %d", r);
    PgScene *root = scenes[0];
    const size_t strayBytes = sizeof(PgStraySample) * (size_t)(maxStrays > 0 ? maxStrays : 1);
    std::vector<PgRenderDesc> rd((size_t)n, *desc);
    std::vector<size_t> filmBytes((size_t)n);
    size_t filmMax = sizeof(PgFilmPixel);  // never an empty buffer, also when no rank owns a tile
    for (int r = 0; r < n; ++r) {
        rd[r].tile_first = r; rd[r].tile_step = n;
        filmBytes[r] = sizeof(PgFilmPixel) * (size_t)desc->tile_pixels * (size_t)pgTileCount(&rd[r]);
        filmMax = std::max(filmMax, filmBytes[r]);
        // a rank that owns no tile (more devices than tiles: a small image or crop window) has nothing to receive: its film
        // pointer may be null; it still runs pg_render (which handles an empty shard) so that its counters and stray count are set
        if (filmBytes[r] && !film[r]) return setError(PG_ERR_INVALID, "pg_render_sharded: null film buffer for rank %d", r);
    }
    // one packed shard per rank, the same size for all: [film (filmMax) | strays | count]; the gathered frame is n of them in rank order
    const size_t strayOff = filmMax, countOff = strayOff + strayBytes, per = (countOff + sizeof(int) + 255) / 256 * 256;
    const size_t total = per * (size_t)n;
    // one sharded render at a time per DEVICE: the communicators of a device list carry one collective at a time and the scenes' shard / gather
    // buffers are per scene, so two calls that share a device wait for each other; calls over disjoint device sets run side by side.  The
    // devices' locks are taken in ascending order of the device number (no two calls can hold them crosswise).
    static std::mutex deviceMutex[64];
    std::vector<int> lockOrder;
    for (int r = 0; r < n; ++r) lockOrder.push_back(scenes[r]->device & 63);
    std::sort(lockOrder.begin(), lockOrder.end());
    lockOrder.erase(std::unique(lockOrder.begin(), lockOrder.end()), lockOrder.end());
    std::vector<std::unique_lock<std::mutex>> deviceLocks;
    for (int dev : lockOrder) deviceLocks.emplace_back(deviceMutex[dev]);
    HIP_TRY(hipSetDevice(root->device));
    if (root->gatherDev.bytes < total) HIP_TRY(root->gatherDev.alloc(total));  // kept between frames (hipFree + hipMalloc synchronise the device)
    char *gather = (char *)root->gatherDev.p;
    // transport: RCCL unless PG_SHARD_GATHER=peer, a device repeats (tests on a one-GPU box) or librccl cannot be used -- then peer copies
    std::string why;
#ifndef HIP_EMU_H
    const std::vector<PgNcclComm> *comms = nullptr;
    {
        const char *e = getenv("PG_SHARD_GATHER");
        std::vector<int> devices((size_t)n);
        for (int r = 0; r < n; ++r) devices[r] = scenes[r]->device;
        if (e && !strcmp(e, "peer")) why = "PG_SHARD_GATHER=peer";
        else comms = shardComms(devices, why);
        if (!comms && e && !strcmp(e, "rccl")) return setError(PG_ERR_DEVICE, "pg_render_sharded: PG_SHARD_GATHER=rccl, but %s", why.c_str());
    }
#else
    why = "emulated devices";
#endif
    std::vector<int> status((size_t)n, PG_OK);
    std::vector<std::string> message((size_t)n);
    // Every rank reaches the collective or none does: a rank whose render failed (out of memory on one device, say) must not leave
    // the other n - 1 threads waiting in ncclGather for a peer that already returned.  The threads meet at a host barrier between
    // the render and the gather; if any of them failed by then, all skip the gather and the caller gets that rank's error.
    struct { std::mutex m; std::condition_variable cv; int arrived = 0; bool anyFailed = false; } meet;
    auto meetAll = [&](bool failed) -> bool {  // returns whether any rank failed
        std::unique_lock<std::mutex> lock(meet.m);
        meet.anyFailed = meet.anyFailed || failed;
        if (++meet.arrived == n) meet.cv.notify_all();
        else meet.cv.wait(lock, [&] { return meet.arrived == n; });
        return meet.anyFailed;
    };
    auto render = [&](int r) -> bool {  // this rank's tiles into its packed shard; false = failed (status / message set)
        PgScene *s = scenes[r];
        if (hipSetDevice(s->device) != hipSuccess) { status[r] = PG_ERR_DEVICE; message[r] = "hipSetDevice failed"; return false; }
        bool viaRccl = false;
#ifndef HIP_EMU_H
        viaRccl = comms != nullptr;
#endif
        if (!viaRccl && s->device != root->device) {  // direct xGMI writes into the gathering device's buffer
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, s->device, root->device) == hipSuccess && can) {
                hipError_t e = hipDeviceEnablePeerAccess(root->device, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { status[r] = PG_ERR_DEVICE; message[r] = hipGetErrorString(e); return false; }
                (void)hipGetLastError();
            }
        }
#ifdef PG_TEST_HOOKS  // fault injection for tests/test_emulated_device.py: compiled into the emulated test build only, never into libpbrt_gpu.so
        if (const char *e = getenv("PG_TEST_FAIL_RANK")) if (atoi(e) == r) { status[r] = PG_ERR_DEVICE; message[r] = "PG_TEST_FAIL_RANK (a test's injected failure)"; return false; }
#endif
        if (s->shardFilm.bytes < per && s->shardFilm.alloc(per) != hipSuccess) { status[r] = PG_ERR_DEVICE; message[r] = "out of device memory (packed shard)"; return false; }
        char *packed = (char *)s->shardFilm.p;
        int st = pg_render(s, &rd[r], (PgFilmPixel *)packed, (PgStraySample *)(packed + strayOff), maxStrays, (int32_t *)(packed + countOff), PG_MEM_DEVICE, nullptr);
        if (st != PG_OK) { status[r] = st; message[r] = pg_last_error(); return false; }
        return true;
    };
    auto work = [&](int r) {
        const bool ok = render(r);
        if (meetAll(!ok)) return;  // some rank failed: nobody enters the collective
        PgScene *s = scenes[r];
        char *packed = (char *)s->shardFilm.p;
#ifndef HIP_EMU_H
        if (comms) {
            // one collective per frame: every rank's thread calls it on its own communicator (the threads are the "different
            // threads" of rccl.h:213); root 0 receives rank r's shard at gather + r * per
            const int rs = rcclApi()->Gather(packed, r == 0 ? gather : nullptr, per, /*ncclChar*/ 0, 0, (*comms)[r], nullptr);
            if (rs != 0) { status[r] = PG_ERR_DEVICE; message[r] = std::string("ncclGather: ") + rcclApi()->GetErrorString(rs); return; }
            const hipError_t e = hipStreamSynchronize(nullptr);
            if (e != hipSuccess) { status[r] = PG_ERR_DEVICE; message[r] = std::string("after ncclGather: ") + hipGetErrorString(e); }
            return;
        }
#endif
        const hipError_t e = hipMemcpyPeer(gather + per * (size_t)r, root->device, packed, s->device, per);
        if (e != hipSuccess) { status[r] = PG_ERR_DEVICE; message[r] = std::string("peer copy of the film shard: ") + hipGetErrorString(e); }
    };
    {
        std::vector<std::thread> threads;
        for (int r = 1; r < n; ++r) threads.emplace_back(work, r);
        work(0);
        for (auto &t : threads) t.join();
    }
    for (int r = 0; r < n; ++r) if (status[r] != PG_OK) return setError(status[r], "rank %d: %s", r, message[r].c_str());
    { std::lock_guard<std::mutex> lock(g_shardTransportMutex); g_shardTransport = why.empty() ? "rccl" : "peer (" + why + ")"; }
    // the gathered frame back to the host in one piece
    HIP_TRY(hipSetDevice(root->device));
    std::vector<char> host(total);
    HIP_TRY(hipMemcpy(host.data(), gather, total, hipMemcpyDeviceToHost));
    for (int r = 0; r < n; ++r) {
        const char *shard = host.data() + per * (size_t)r;
        if (filmBytes[r]) memcpy(film[r], shard, filmBytes[r]);
        int cnt = 0;
        memcpy(&cnt, shard + countOff, sizeof(int));
        cnt = std::max(0, std::min(cnt, (int)maxStrays));
        if (cnt > 0) memcpy(strays[r], shard + strayOff, sizeof(PgStraySample) * (size_t)cnt);
        nStrays[r] = cnt;
    }
    return PG_OK;
}

// ---- the batched queries --------------------------------------------------------------
// pg_intersect / pg_intersect_p (rays at time 0; primitive, t and barycentrics), pg_intersect_at / pg_intersect_p_at (Ray::time; the
// SurfaceInteraction, pg_interaction.h), pg_scatter_f_at / pg_scatter_sample_at (the BSDF at the closest hit, pg_scatter.h) and pg_light_le_at (the
// radiance the ray meets, pg_lightquery.h) are one device path, rayQuery: pack, trace, emit, account, one wait.  The other families have a driver each:
// lightQuery (reference points instead of rays), mediumQuery, subsurfaceQuery with adapterQuery, pg_camera_rays_at, and pg_camera_we_at /
// pg_camera_sample_wi_at.  What the drivers share is
// stated once, in front of them:
//   checkArgs    the entry points' refusals
//   Staging      a call's host arrays <-> the scene's two staging arenas
//   queryScene   the scene as pg_intersect_at's launch sees it
//   queueOver    a RayQueue over grow-only buffers (testQueue: the test queue; packRays: ... with the call's rays in it)
//   finishQuery  the call's one wait, its counters, the cull guard
// and, with the renderer, queueSize and sssProbeChains above.
// The queries' buffers only grow: DeviceBuffer::alloc frees first, and hipFree waits for the device
static hipError_t reserve(DeviceBuffer &b, size_t bytes) { return b.bytes >= bytes ? hipSuccess : b.alloc(bytes); }

// The refusals, in this order: no scene, n < 0 or -- of a call with work to do -- a required array missing; `flags` that are no BxDFType mask (the
// scattering calls pass theirs).  n == 0 is the caller's to return PG_OK for, before anything is dereferenced or the device is touched
static int checkArgs(const char *name, const PgScene *s, int32_t n, std::initializer_list<const void *> required, int32_t flags = 0) {
    bool refused = !s || n < 0;
    if (n > 0) for (const void *p : required) refused = refused || !p;
    if (refused) return setError(PG_ERR_INVALID, "%s: null argument", name);
    if (flags < 0 || flags > 31) return setError(PG_ERR_INVALID, "%s: flags %d is not a BxDFType mask (0 .. 31)", name, flags);
    return PG_OK;
}

extern "C++" {  // (templates)
// A call's arrays in the caller's memory and what the kernels use in their place.  The driver declares its inputs and outputs -- in() / out(): its
// pointer variable and the array's element count; an array that is not given (nullptr) takes no part -- and upload() re-aims the declared variables.
// PG_MEM_DEVICE: nothing is declared or copied, the kernels read and write the caller's arrays.  Otherwise each array gets a slot on a 16-byte boundary
// (PgInteraction, PgCameraRay and the differentials are read or written as float4) of PgScene::stageIn or stageOut, upload() enqueues the inputs'
// copies and download() the results'; the host arrays must outlive the stream's work, which the entry points wait for before they return.
// Both arenas are grown for the whole call before its first copy is enqueued: growing frees the old block, which no work of this call may be using.
struct Staging {
    PgScene *s; hipStream_t stream; bool device;
    struct Slot { void *var, *host; size_t bytes, offset; };  // (var: the driver's pointer variable)
    std::vector<Slot> ins, outs;
    size_t inBytes = 0, outBytes = 0;
    Staging(PgScene *s, int mem, hipStream_t stream) : s(s), stream(stream), device(mem == PG_MEM_DEVICE) {}
    static void add(std::vector<Slot> &slots, size_t &total, void *var, void *host, size_t bytes) {
        slots.push_back({var, host, bytes, total});
        total += (bytes + 15) & ~(size_t)15;
    }
    template <class T> void in(const T *&p, size_t count) {
        if (device || !p) return;
        if (count) add(ins, inBytes, &p, const_cast<T *>(p), count * sizeof(T));
        else p = nullptr;  // (draws of a call with n_u = 0: nothing to read)
    }
    template <class T> void out(T *&p, size_t count) { if (!device && p) add(outs, outBytes, &p, p, count * sizeof(T)); }
    // o, d (three floats per ray), tmax and -- where given -- time
    void rays(const float *&o, const float *&d, const float *&tmax, const float *&time, size_t n) { in(o, 3 * n); in(d, 3 * n); in(tmax, n); in(time, n); }
    int upload() {
        HIP_TRY(reserve(s->stageIn, inBytes));
        HIP_TRY(reserve(s->stageOut, outBytes));
        for (const Slot &t : ins) {
            void *dev = (char *)s->stageIn.p + t.offset;
            HIP_TRY(hipMemcpyAsync(dev, t.host, t.bytes, hipMemcpyHostToDevice, stream));
            memcpy(t.var, &dev, sizeof(dev));
        }
        for (const Slot &t : outs) {
            void *dev = (char *)s->stageOut.p + t.offset;
            memcpy(t.var, &dev, sizeof(dev));
        }
        return PG_OK;
    }
    int download() {
        for (const Slot &t : outs) HIP_TRY(hipMemcpyAsync(t.host, (char *)s->stageOut.p + t.offset, t.bytes, hipMemcpyDeviceToHost, stream));
        return PG_OK;
    }
};
}  // extern "C++"

// The scene as pg_intersect_at's launch sees it -- as a frame's: the hits' instances, a moving one's matrices at the ray's time -- over the queries' own
// records for `entries` hits.  dsc: a copy of s->d
static int queryScene(PgScene *s, size_t entries, DScene &dsc) {
    dsc.hitInst = nullptr; dsc.animXf = nullptr; dsc.nestXfOff = 0;
    if (dsc.nInstances > 0) { HIP_TRY(reserve(s->tInst, sizeof(int) * entries)); dsc.hitInst = (int *)s->tInst.p; }
    if (dsc.hasMotion) {
        HIP_TRY(reserve(s->tXf, (dsc.hasNest ? 2 : 1) * entries * PG_XF_STRIDE * sizeof(float)));  // (hasNest: a second half for the inner transform)
        dsc.animXf = (float *)s->tXf.p; dsc.nestXfOff = (int)entries;
    }
    return PG_OK;
}
// A queue of PG_REGIONS regions of `cap` entries over the buffers o and d with the counter block `counts`, its rays' times behind `d` in
// PG_QUEUE_TIMES's layout -- for every scene: a still scene's k_trace does not read them, the records report them
static int queueOver(DeviceBuffer &o, DeviceBuffer &d, int *counts, int cap, RayQueue &q, float *&times) {
    const size_t N = (size_t)cap * PG_REGIONS;
    HIP_TRY(reserve(o, N * sizeof(float4)));
    HIP_TRY(reserve(d, N * (sizeof(float4) + sizeof(float))));
    q.o = (float4 *)o.p; q.d = (float4 *)d.p; q.counts = counts; q.regionCap = cap;
    times = reinterpret_cast<float *>(q.d + N);
    return PG_OK;
}
static int testQueue(PgScene *s, int cap, RayQueue &q, float *&times) {
    HIP_TRY(reserve(s->tCount, QSTRIDE * sizeof(int)));
    return queueOver(s->tO, s->tD, (int *)s->tCount.p, cap, q, times);
}
// The rays (in device memory: staged by the driver) into the test queue ON the device (k_pack_rays): ray i at entry i
static int packRays(PgScene *s, int n, const float *o, const float *d, const float *tmax, const float *time, hipStream_t stream, RayQueue &q, float *&times) {
    if (int e = testQueue(s, regionCapFor(n), q, times)) return e;
    launch_pack_rays(o, d, tmax, time, n, q, times, stream);
    return PG_OK;
}
// The end of a call that traced.  Behind the call's work it reads the device's trace totals (tc[0] closest hit, tc[1] any hit), a closest-hit call's
// cull guard -- only such a launch can raise it, and it decides whether the results stand -- and, rayCounts != nullptr, that queue's counters: its size
// is then the number of rays (pg_light_sample_at: the sample kernel chose the rays to test).  The call's one wait (the walks' per-pass waits aside);
// then the call's rays and launches join the scene's counters, with the totals of a call that launched and the time between the events a and b of a
// driver that recorded them around its one launch
static int finishQuery(PgScene *s, hipStream_t stream, bool anyhit, uint64_t rays, uint64_t launches, hipEvent_t a = nullptr, hipEvent_t b = nullptr,
                       const int *rayCounts = nullptr) {
    TraceCounters tc[2];
    int guard = 0, blk[QSTRIDE];
    HIP_TRY(hipMemcpyAsync(tc, s->traceCn.p, sizeof(tc), hipMemcpyDeviceToHost, stream));
    if (!anyhit) HIP_TRY(hipMemcpyAsync(&guard, s->cullGuard.p, sizeof(int), hipMemcpyDeviceToHost, stream));
    if (rayCounts) HIP_TRY(hipMemcpyAsync(blk, rayCounts, sizeof(blk), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (rayCounts) rays = queueTotal(blk, 0);
    PgCounters &c = s->counters;
    (anyhit ? c.shadow_rays : c.closest_rays) += rays;
    (anyhit ? c.shadow_launches : c.closest_launches) += launches;
    if (launches) {
        (anyhit ? c.shadow_node_visits : c.closest_node_visits) = tc[anyhit].node_visits;
        (anyhit ? c.shadow_tri_tests : c.closest_tri_tests) = tc[anyhit].tri_tests;
        c.node_visits = tc[0].node_visits + tc[1].node_visits;
        c.tri_tests = tc[0].tri_tests + tc[1].tri_tests + c.light_tri_tests;
    }
    float ms = 0;
    if (a && hipEventElapsedTime(&ms, a, b) == hipSuccess) (anyhit ? c.shadow_ms : c.closest_ms) += ms;
    return cullGuardStatus(s, guard);
}

// One call of the seven entry points: the rays, and the caller's arrays (in `mem`) of the kind of result it asks for
struct RayQuery {
    int32_t n;
    const float *o, *d, *tmax, *time;  // time == nullptr: every ray at time 0
    bool anyhit;                       // Scene::IntersectP
    bool at;                           // the _at pair: the rays' times count, a closest hit's record is the PgInteraction
    int32_t *prim; float *t, *bary;    // pg_intersect
    PgInteraction *out;                // pg_intersect_at; the scattering queries' and pg_light_le_at's `isect` (may be nullptr there)
    uint8_t *occluded;                 // pg_intersect_p, pg_intersect_p_at
    int mem;
    void *stream;
    // the scattering queries (at, not anyhit): scatter != nullptr, the records; scatterIn = wi (three floats per ray) or -- sample -- u (two)
    PgScatter *scatter = nullptr;
    const float *scatterIn = nullptr;
    bool sample = false;
    int32_t flags = 0;
    float *le = nullptr;  // pg_light_le_at (at, not anyhit): three floats per ray
    const float *diff = nullptr;  // pg_scatter_*_diff_at: the rays' differentials, twelve floats per ray (nullptr: rays without)
    bool importance = false;      // pg_scatter_*_mode_at with mode 1: the BSDF of TransportMode::Importance (pg_cameraimportance.h)
};
static int rayQuery(PgScene *s, RayQuery r) {
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = (hipStream_t)r.stream;
    const size_t n = (size_t)r.n;
    // (a scattering query's differentials, pg_cameraquery.h, are read by scenes with textured materials or nesting alone: the rest take the plain kernel)
    if (!s->d.hasTextured && !s->d.hasNest) r.diff = nullptr;
    Staging stage(s, r.mem, stream);
    stage.rays(r.o, r.d, r.tmax, r.time, n);
    stage.in(r.scatterIn, (r.sample ? 2 : 3) * n);
    stage.in(r.diff, 12 * n);
    stage.out(r.scatter, n); stage.out(r.out, n); stage.out(r.le, 3 * n);
    stage.out(r.prim, n); stage.out(r.t, n); stage.out(r.bary, 3 * n);
    stage.out(r.occluded, n);
    if (int e = stage.upload()) return e;
    RayQueue q;
    float *times = nullptr;
    if (int e = packRays(s, r.n, r.o, r.d, r.tmax, r.time, stream, q, times)) return e;
    // --- the scene and the tunables the launch sees, per entry point:
    //   pg_intersect       no instance or matrix records (primitive, t and barycentrics are all it reports); rays at time 0
    //   pg_intersect_p     rays at time 0 (an any-hit launch touches neither record)
    //   pg_intersect_at    queryScene, the records by ray
    //   pg_scatter_*_at, pg_light_le_at  as pg_intersect_at
    //   pg_intersect_p_at  no records; the rays' times as the scene has them
    // any hit: in the reference's visiting order, so that the counters are the reference's (tests compare them)
    DScene dsc = s->d;
    TraceConfig cfg = s->trace;
    if (!r.at) dsc.rayTimes = 0;
    if (r.anyhit) cfg.anyhitFree = 0;
    if (r.at && !r.anyhit) { if (int e = queryScene(s, n, dsc)) return e; }
    else { dsc.hitInst = nullptr; dsc.animXf = nullptr; }
    if (r.anyhit) HIP_TRY(reserve(s->tOcc, sizeof(int) * n));
    else { HIP_TRY(reserve(s->tHit, sizeof(float4) * n)); HIP_TRY(reserve(s->tT, sizeof(float) * n)); }
    // --- the differentials reach k_scatter_diff by ray, through a LensFrame of this call's in front of `stL`, the way a realistic camera's frame keeps them by slot
    const float4 *stL = nullptr;
    if (r.diff) {
        HIP_TRY(reserve(s->cqFrame, PG_LENS_FRAME_BYTES));
        s->cqHead = LensFrame{};
        s->cqHead.differentials = reinterpret_cast<float4 *>(const_cast<float *>(r.diff));
        HIP_TRY(hipMemcpyAsync(s->cqFrame.p, &s->cqHead, sizeof(LensFrame), hipMemcpyHostToDevice, stream));
        stL = reinterpret_cast<const float4 *>((const char *)s->cqFrame.p + PG_LENS_FRAME_BYTES);  // (an address only: nothing is read at or behind it)
    }
    hipEvent_t a = getEvent(s, 0), b = getEvent(s, 1);
    HIP_TRY(hipEventRecord(a, stream));
    if (r.anyhit) launch_anyhit(dsc, cfg, q, (int *)s->tOcc.p, (TraceCounters *)s->traceCn.p + 1, (int *)s->cursors.p, stream);
    else launch_closest(dsc, cfg, q, (float4 *)s->tHit.p, (float *)s->tT.p, (TraceCounters *)s->traceCn.p, (int *)s->cursors.p, (int *)s->cullGuard.p, stream);
    HIP_TRY(hipEventRecord(b, stream));
    if (r.anyhit) launch_occluded_bytes((const int *)s->tOcc.p, r.occluded, r.n, stream);
    else if (r.at) {
        if (r.scatter && r.importance) launch_scatter_importance(dsc, q, (const float4 *)s->tHit.p, r.scatterIn, r.sample, r.flags, stL, r.scatter, stream);
        else if (r.scatter && stL) launch_scatter_diff(dsc, q, (const float4 *)s->tHit.p, r.scatterIn, r.sample, r.flags, stL, r.scatter, stream);
        else if (r.scatter) launch_scatter(dsc, q, (const float4 *)s->tHit.p, r.scatterIn, r.sample, r.flags, r.scatter, stream);
        if (r.out) launch_interaction(dsc, q, (const float4 *)s->tHit.p, (const float *)s->tT.p, times, r.out, stream);
        if (r.le) launch_emitted(dsc, q, (const float4 *)s->tHit.p, r.le, stream);
    }
    else launch_hit_arrays((const float4 *)s->tHit.p, (const float *)s->tT.p, r.prim, r.t, r.bary, r.n, stream);
    HIP_TRY(hipGetLastError());
    if (int e = stage.download()) return e;
    return finishQuery(s, stream, r.anyhit, n, 1, a, b);
}

int pg_intersect(PgScene *s, int32_t n, const float *o, const float *d, const float *tmax, int32_t *prim, float *t, float *bary, int mem,
                 void *streamPtr) {
    if (int e = checkArgs("pg_intersect", s, n, {o, d, tmax, prim, t, bary})) return e;
    if (n == 0) return PG_OK;
    const RayQuery r = {n, o, d, tmax, nullptr, false, false, prim, t, bary, nullptr, nullptr, mem, streamPtr};
    return withExactFallback(s, [&]() { return rayQuery(s, r); });
}
int pg_intersect_p(PgScene *s, int32_t n, const float *o, const float *d, const float *tmax, uint8_t *occluded, int mem, void *streamPtr) {
    if (int e = checkArgs("pg_intersect_p", s, n, {o, d, tmax, occluded})) return e;
    if (n == 0) return PG_OK;
    return rayQuery(s, {n, o, d, tmax, nullptr, true, false, nullptr, nullptr, nullptr, nullptr, occluded, mem, streamPtr});
}
int pg_intersect_at(PgScene *s, int32_t n, const float *o, const float *d, const float *tmax, const float *time, PgInteraction *out, int mem,
                    void *streamPtr) {
    if (int e = checkArgs("pg_intersect_at", s, n, {o, d, tmax, out})) return e;
    if (n == 0) return PG_OK;
    const RayQuery r = {n, o, d, tmax, time, false, true, nullptr, nullptr, nullptr, out, nullptr, mem, streamPtr};
    return withExactFallback(s, [&]() { return rayQuery(s, r); });
}
int pg_intersect_p_at(PgScene *s, int32_t n, const float *o, const float *d, const float *tmax, const float *time, uint8_t *occluded, int mem,
                      void *streamPtr) {
    if (int e = checkArgs("pg_intersect_p_at", s, n, {o, d, tmax, occluded})) return e;
    if (n == 0) return PG_OK;
    return rayQuery(s, {n, o, d, tmax, time, true, true, nullptr, nullptr, nullptr, nullptr, occluded, mem, streamPtr});
}
// The two scattering queries: pg_intersect_at's call with the BSDF's records beside (or instead of) the interactions
static int scatterQuery(const char *name, PgScene *s, int32_t n, const float *o, const float *d, const float *tmax, const float *time, const float *in, bool sample,
                        int32_t flags, PgInteraction *isect, PgScatter *out, int mem, void *streamPtr, const float *diff = nullptr, int32_t mode = 0) {
    if (int e = checkArgs(name, s, n, {o, d, tmax, in, out}, flags)) return e;
    if (mode < 0 || mode > 1) return setError(PG_ERR_INVALID, "%s: mode %d is no TransportMode (0 = Radiance, 1 = Importance)", name, mode);
    if (diff && mem == PG_MEM_DEVICE && ((uintptr_t)diff & 15)) return setError(PG_ERR_INVALID, "%s: diff in device memory must be 16-byte aligned (it is read as float4)", name);
    if (n == 0) return PG_OK;
    RayQuery r = {n, o, d, tmax, time, false, true, nullptr, nullptr, nullptr, isect, nullptr, mem, streamPtr};
    r.scatter = out; r.scatterIn = in; r.sample = sample; r.flags = flags; r.diff = diff; r.importance = mode == 1;
    return withExactFallback(s, [&]() { return rayQuery(s, r); });
}
int pg_scatter_f_at(PgScene *s, int32_t n, const float *o, const float *d, const float *tmax, const float *time, const float *wi, int32_t flags,
                    PgInteraction *isect, PgScatter *out, int mem, void *streamPtr) {
    return scatterQuery("pg_scatter_f_at", s, n, o, d, tmax, time, wi, false, flags, isect, out, mem, streamPtr);
}
int pg_scatter_sample_at(PgScene *s, int32_t n, const float *o, const float *d, const float *tmax, const float *time, const float *u, int32_t flags,
                         PgInteraction *isect, PgScatter *out, int mem, void *streamPtr) {
    return scatterQuery("pg_scatter_sample_at", s, n, o, d, tmax, time, u, true, flags, isect, out, mem, streamPtr);
}
// The same two for rays with differentials (diff == nullptr: the plain calls)
int pg_scatter_f_diff_at(PgScene *s, int32_t n, const float *o, const float *d, const float *tmax, const float *time, const float *wi, const float *diff, int32_t flags,
                         PgInteraction *isect, PgScatter *out, int mem, void *streamPtr) {
    return scatterQuery("pg_scatter_f_diff_at", s, n, o, d, tmax, time, wi, false, flags, isect, out, mem, streamPtr, diff);
}
int pg_scatter_sample_diff_at(PgScene *s, int32_t n, const float *o, const float *d, const float *tmax, const float *time, const float *u, const float *diff, int32_t flags,
                              PgInteraction *isect, PgScatter *out, int mem, void *streamPtr) {
    return scatterQuery("pg_scatter_sample_diff_at", s, n, o, d, tmax, time, u, true, flags, isect, out, mem, streamPtr, diff);
}
// ... and under a TransportMode: 0 = Radiance, the calls above; 1 = Importance, the same device path with launch_scatter_importance's kernel
int pg_scatter_f_mode_at(PgScene *s, int32_t n, const float *o, const float *d, const float *tmax, const float *time, const float *wi, const float *diff, int32_t flags,
                         int32_t mode, PgInteraction *isect, PgScatter *out, int mem, void *streamPtr) {
    return scatterQuery("pg_scatter_f_mode_at", s, n, o, d, tmax, time, wi, false, flags, isect, out, mem, streamPtr, diff, mode);
}
int pg_scatter_sample_mode_at(PgScene *s, int32_t n, const float *o, const float *d, const float *tmax, const float *time, const float *u, const float *diff, int32_t flags,
                              int32_t mode, PgInteraction *isect, PgScatter *out, int mem, void *streamPtr) {
    return scatterQuery("pg_scatter_sample_mode_at", s, n, o, d, tmax, time, u, true, flags, isect, out, mem, streamPtr, diff, mode);
}
int pg_light_le_at(PgScene *s, int32_t n, const float *o, const float *d, const float *tmax, const float *time, PgInteraction *isect, float *Le, int mem,
                   void *streamPtr) {
    if (int e = checkArgs("pg_light_le_at", s, n, {o, d, tmax, Le})) return e;
    if (n == 0) return PG_OK;
    RayQuery r = {n, o, d, tmax, time, false, true, nullptr, nullptr, nullptr, isect, nullptr, mem, streamPtr};
    r.le = Le;
    return withExactFallback(s, [&]() { return rayQuery(s, r); });
}

// ---- batched Camera::GenerateRayDifferential (pg_cameraquery.h) ----
// Check, stage, one launch, copy back, one wait.  The description is checked as a frame's is (pg_check_render_desc) before the device is touched -- first by
// itself, over facts that grant whatever it asks of a scene (the camera's kind and lens tables index the device's code and need no scene), then against this scene's.
// The realistic camera's lens block and zeroed statistics go into the call's LensFrame, whose counts are added to the scene's counters as a frame's are
// (camera_rays excepted: no ray is traced)
static int checkCameraDescAlone(const PgRenderDesc *&rd, PgRenderDesc &current) {
    rd = pgCurrentRenderDesc(rd, current);
    std::string err;
    RenderSceneFacts granted = {INT_MAX, true, true, true, INT_MAX};
    if (int st = pg_check_render_desc(rd, granted, err)) return setError(st, "%s", err.c_str());
    return PG_OK;
}
static int checkCameraDescOfScene(const PgScene *s, const PgRenderDesc *rd) {
    std::string err;
    const RenderSceneFacts facts = {s->nMedia, s->cmaxmin.p != nullptr, s->d.sobolMatrices != nullptr, s->d.perms != nullptr, s->d.nPermDims};
    if (int st = pg_check_render_desc(rd, facts, err)) return setError(st, "%s", err.c_str());
    return PG_OK;
}
int pg_camera_rays_at(PgScene *s, const PgRenderDesc *rd, int32_t n, const float *pFilm, const float *pLens, const float *uTime, PgCameraRay *out, int mem,
                      void *streamPtr) {
    if (int e = checkArgs("pg_camera_rays_at", rd ? s : nullptr, n, {pFilm, out})) return e;  // (the description is required as the scene is, whatever n)
    if (n == 0) return PG_OK;
    PgRenderDesc current;
    if (int e = checkCameraDescAlone(rd, current)) return e;
    if (int e = checkCameraDescOfScene(s, rd)) return e;
    if (mem == PG_MEM_DEVICE && ((uintptr_t)out & 15)) return setError(PG_ERR_INVALID, "pg_camera_rays_at: out in device memory must be 16-byte aligned (it is written as float4)");
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = (hipStream_t)streamPtr;
    const size_t N = (size_t)n;
    Staging stage(s, mem, stream);
    stage.in(pFilm, 2 * N); stage.in(pLens, 2 * N); stage.in(uTime, N);
    stage.out(out, N);
    if (int e = stage.upload()) return e;
    LensFrame *lf = nullptr;
    if (rd->camera_type == 3) {
        HIP_TRY(reserve(s->cqFrame, PG_LENS_FRAME_BYTES));
        s->cqHead = LensFrame{};
        memcpy(&s->cqHead.lens, &rd->n_lens_interfaces, sizeof(PgLensSystem));
        HIP_TRY(hipMemcpyAsync(s->cqFrame.p, &s->cqHead, sizeof(LensFrame), hipMemcpyHostToDevice, stream));
        lf = (LensFrame *)s->cqFrame.p;
    }
    launch_camera_rays(*rd, lf, pFilm, pLens, uTime, n, out, stream);
    HIP_TRY(hipGetLastError());
    if (int e = stage.download()) return e;
    unsigned long long ls[3] = {0, 0, 0};
    if (lf) HIP_TRY(hipMemcpyAsync(ls, (const char *)lf + offsetof(LensFrame, stats), sizeof(ls), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));  // the call's one wait
    s->counters.lens_rays_total += ls[0]; s->counters.lens_rays_vignetted += ls[1];
    return PG_OK;
}

// ---- batched Light::Sample_Li + VisibilityTester::Unoccluded, and Light::Pdf_Li, at reference points ----
// One call of pg_light_sample_at (out != nullptr: u, two floats per sample) or pg_light_pdf_at (pdf != nullptr: wi, three)
struct LightQuery {
    int32_t n;
    const PgInteraction *ref;
    const int32_t *light;
    const float *in;
    PgLightSample *out; float *shadow;  // pg_light_sample_at (shadow may be nullptr: else eight floats per sample)
    float *pdf;                         // pg_light_pdf_at
    int mem;
    void *stream;
};
// Stage, sample, trace, visibility, copy back, one wait.  The sample kernel appends the rays of the samples EstimateDirect would test to the test
// queue; the any-hit launch sees the scene as pg_intersect_p_at's does (the rays' times as the scene has them, the reference's visiting order).
// pg_light_pdf_at traces nothing and moves no counter
static int lightQuery(PgScene *s, LightQuery r) {
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = (hipStream_t)r.stream;
    const size_t n = (size_t)r.n;
    const bool sample = r.out != nullptr;
    Staging stage(s, r.mem, stream);
    stage.in(r.ref, n); stage.in(r.in, (sample ? 2 : 3) * n); stage.in(r.light, n);
    stage.out(r.out, n); stage.out(r.shadow, 8 * n); stage.out(r.pdf, n);
    if (int e = stage.upload()) return e;
    DScene dsc = s->d;
    dsc.hitInst = nullptr; dsc.animXf = nullptr;
    if (!sample) {
        launch_light_pdf(dsc, r.ref, r.light, r.in, r.n, r.pdf, stream);
        HIP_TRY(hipGetLastError());
        if (int e = stage.download()) return e;
        HIP_TRY(hipStreamSynchronize(stream));
        return PG_OK;
    }
    // the test queue, empty: k_light_sample appends to it
    RayQueue q;
    float *times = nullptr;
    if (int e = testQueue(s, regionCapFor(r.n), q, times)) return e;
    HIP_TRY(reserve(s->tOcc, sizeof(int) * (size_t)q.regionCap * PG_REGIONS));  // (answers by queue entry: the regions are not filled front to back here)
    HIP_TRY(hipMemsetAsync(q.counts, 0, QSTRIDE * sizeof(int), stream));
    launch_light_sample(dsc, r.ref, r.light, r.in, r.n, q, times, r.out, r.shadow, stream);
    TraceConfig cfg = s->trace;
    cfg.anyhitFree = 0;
    hipEvent_t a = getEvent(s, 0), b = getEvent(s, 1);
    HIP_TRY(hipEventRecord(a, stream));
    launch_anyhit(dsc, cfg, q, (int *)s->tOcc.p, (TraceCounters *)s->traceCn.p + 1, (int *)s->cursors.p, stream);
    HIP_TRY(hipEventRecord(b, stream));
    launch_light_visibility(q, (const int *)s->tOcc.p, r.out, stream);
    HIP_TRY(hipGetLastError());
    if (int e = stage.download()) return e;
    return finishQuery(s, stream, true, 0, 1, a, b, q.counts);
}
int pg_light_sample_at(PgScene *s, int32_t n, const PgInteraction *ref, const int32_t *light, const float *u, PgLightSample *out, float *shadow, int mem,
                       void *streamPtr) {
    if (int e = checkArgs("pg_light_sample_at", s, n, {ref, light, u, out})) return e;
    if (n == 0) return PG_OK;
    return lightQuery(s, {n, ref, light, u, out, shadow, nullptr, mem, streamPtr});
}
int pg_light_pdf_at(PgScene *s, int32_t n, const PgInteraction *ref, const int32_t *light, const float *wi, float *pdf, int mem, void *streamPtr) {
    if (int e = checkArgs("pg_light_pdf_at", s, n, {ref, light, wi, pdf})) return e;
    if (n == 0) return PG_OK;
    return lightQuery(s, {n, ref, light, wi, nullptr, nullptr, pdf, mem, streamPtr});
}

// ---- batched Camera::We / Pdf_We and Camera::Sample_Wi + VisibilityTester::Unoccluded (pg_cameraimportance.h) ----
// The refusals of both calls, before the device is touched: arguments, a camera that is not the perspective one (the description is checked by itself first,
// so that a camera without We answers PG_ERR_UNSUPPORTED on any scene), `we`, the description against the scene, a misaligned device output
static int cameraWeArgs(const char *name, PgScene *s, const PgRenderDesc *&rd, PgRenderDesc &current, const PgCameraWeDesc *we, int32_t n,
                        std::initializer_list<const void *> required, const void *out, int mem) {
    if (int e = checkArgs(name, rd && we ? s : nullptr, n, required)) return e;  // (both descriptions are required as the scene is, whatever n)
    if (n == 0) return PG_OK;
    if (int e = checkCameraDescAlone(rd, current)) return e;
    if (rd->camera_type != 0)
        return setError(PG_ERR_UNSUPPORTED, "%s: camera_type %d -- Camera::We / Pdf_We / Sample_Wi exist for the perspective camera (0) alone", name, rd->camera_type);
    bool finite = std::isfinite(we->image_area);
    for (int k = 0; k < 16; ++k) finite = finite && std::isfinite(we->camera_to_raster[k]) && std::isfinite(we->world_to_camera[k]) && std::isfinite(we->world_to_camera_end[k]);
    if (!finite || !(we->image_area > 0))
        return setError(PG_ERR_INVALID, "%s: PgCameraWeDesc must hold finite matrices and image_area > 0 (image_area %g)", name, (double)we->image_area);
    if (int e = checkCameraDescOfScene(s, rd)) return e;
    if (mem == PG_MEM_DEVICE && ((uintptr_t)out & 15)) return setError(PG_ERR_INVALID, "%s: out in device memory must be 16-byte aligned (it is written as float4)", name);
    return PG_OK;
}
// Check, stage, one launch, copy back, one wait.  Nothing is traced, no counter moves
int pg_camera_we_at(PgScene *s, const PgRenderDesc *rd, const PgCameraWeDesc *we, int32_t n, const float *o, const float *d, const float *time,
                    PgCameraImportance *out, int mem, void *streamPtr) {
    PgRenderDesc current;
    if (int e = cameraWeArgs("pg_camera_we_at", s, rd, current, we, n, {o, d, out}, out, mem)) return e;
    if (n == 0) return PG_OK;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = (hipStream_t)streamPtr;
    const size_t N = (size_t)n;
    Staging stage(s, mem, stream);
    stage.in(o, 3 * N); stage.in(d, 3 * N); stage.in(time, N);
    stage.out(out, N);
    if (int e = stage.upload()) return e;
    launch_camera_we(*rd, *we, o, d, time, n, out, stream);
    HIP_TRY(hipGetLastError());
    if (int e = stage.download()) return e;
    HIP_TRY(hipStreamSynchronize(stream));  // the call's one wait
    return PG_OK;
}
// lightQuery's sample path with the camera's kernel in the light's place: stage, sample (the kernel appends the rays of the samples bdpt would connect to the
// test queue), trace, visibility, copy back, one wait
int pg_camera_sample_wi_at(PgScene *s, const PgRenderDesc *rd, const PgCameraWeDesc *we, int32_t n, const PgInteraction *ref, const float *u,
                           PgCameraSample *out, float *shadow, int mem, void *streamPtr) {
    PgRenderDesc current;
    if (int e = cameraWeArgs("pg_camera_sample_wi_at", s, rd, current, we, n, {ref, u, out}, out, mem)) return e;
    if (n == 0) return PG_OK;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = (hipStream_t)streamPtr;
    const size_t N = (size_t)n;
    Staging stage(s, mem, stream);
    stage.in(ref, N); stage.in(u, 2 * N);
    stage.out(out, N); stage.out(shadow, 8 * N);
    if (int e = stage.upload()) return e;
    DScene dsc = s->d;
    dsc.hitInst = nullptr; dsc.animXf = nullptr;
    RayQueue q;
    float *times = nullptr;
    if (int e = testQueue(s, regionCapFor(n), q, times)) return e;
    HIP_TRY(reserve(s->tOcc, sizeof(int) * (size_t)q.regionCap * PG_REGIONS));  // (answers by queue entry, as lightQuery's)
    HIP_TRY(hipMemsetAsync(q.counts, 0, QSTRIDE * sizeof(int), stream));
    launch_camera_sample_wi(*rd, *we, ref, u, n, q, times, out, shadow, stream);
    TraceConfig cfg = s->trace;
    cfg.anyhitFree = 0;
    hipEvent_t a = getEvent(s, 0), b = getEvent(s, 1);
    HIP_TRY(hipEventRecord(a, stream));
    launch_anyhit(dsc, cfg, q, (int *)s->tOcc.p, (TraceCounters *)s->traceCn.p + 1, (int *)s->cursors.p, stream);
    HIP_TRY(hipEventRecord(b, stream));
    launch_light_visibility(q, (const int *)s->tOcc.p, reinterpret_cast<PgLightSample *>(out), stream);  // (`visibility` lies where PgLightSample has it)
    HIP_TRY(hipGetLastError());
    if (int e = stage.download()) return e;
    return finishQuery(s, stream, true, 0, 1, a, b, q.counts);
}

// ---- batched VisibilityTester::Tr, Scene::IntersectTr and Medium::Sample ----
// One call of pg_transmittance_at (p1 != nullptr), pg_intersect_tr_at (isectTr) or pg_medium_sample_at (sample != nullptr)
struct MediumQuery {
    int32_t n;
    const float *o, *d, *tmax, *time, *p1;
    const int32_t *medium;
    const float *u; int32_t nU;
    PgTransmittance *out;
    bool isectTr; PgInteraction *isect;  // pg_intersect_tr_at (isect may be nullptr)
    PgMediumSample *sample;              // pg_medium_sample_at
    int mem;
    void *stream;
};
// The walks are throughRays' loop over this call's own buffers: packRays fills the test queue, k_tr_seed moves the rays with a valid medium into the
// second queue (mqO / mqD) with their state, then per pass launch_closest -- queryScene, the records by queue entry -- and k_tr_step, which
// finishes rays into their records and appends the re-spawned ones to the other queue; the queue's size is read once per pass.
// pg_medium_sample_at traces nothing and moves no counter
static int mediumQuery(PgScene *s, MediumQuery r) {
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = (hipStream_t)r.stream;
    const size_t n = (size_t)r.n;
    Staging stage(s, r.mem, stream);
    stage.rays(r.o, r.d, r.tmax, r.time, n);
    stage.in(r.p1, 3 * n); stage.in(r.medium, n); stage.in(r.u, n * (size_t)r.nU);
    stage.out(r.sample, n); stage.out(r.out, n); stage.out(r.isect, n);
    if (int e = stage.upload()) return e;
    if (r.sample) {
        launch_medium_sample(s->d, s->nMedia, r.o, r.d, r.tmax, r.medium, r.u, r.nU, r.n, r.sample, stream);
        HIP_TRY(hipGetLastError());
        if (int e = stage.download()) return e;
        HIP_TRY(hipStreamSynchronize(stream));
        return PG_OK;
    }
    // --- the two queues: the test queue (packed: ray i at entry i) and the walk's own
    RayQueue q[2];
    float *times[2];
    if (int e = packRays(s, r.n, r.o, r.d, r.tmax, r.time, stream, q[1], times[1])) return e;
    const int cap = q[1].regionCap;
    const size_t N = (size_t)cap * PG_REGIONS;
    HIP_TRY(reserve(s->mqCount, QSTRIDE * sizeof(int)));
    if (int e = queueOver(s->mqO, s->mqD, (int *)s->mqCount.p, cap, q[0], times[0])) return e;
    // --- the walk's state by ray, a pass's records by entry (the regions are not filled front to back after the first append)
    HIP_TRY(reserve(s->mqState, n * (2 * sizeof(float4) + sizeof(int2))));
    TrState state;
    state.tr = (float4 *)s->mqState.p; state.p1 = state.tr + n; state.cnt = (int2 *)(state.p1 + n);
    HIP_TRY(reserve(s->tHit, sizeof(float4) * N)); HIP_TRY(reserve(s->tT, sizeof(float) * N));
    if (r.isect) HIP_TRY(reserve(s->mqIsect, N * sizeof(PgInteraction)));
    DScene dsc = s->d;
    if (int e = queryScene(s, N, dsc)) return e;
    HIP_TRY(hipMemsetAsync(q[0].counts, 0, QSTRIDE * sizeof(int), stream));
    launch_tr_seed(s->nMedia, q[1], times[1], r.medium, r.p1, r.n, state, q[0], times[0], r.out, r.isect, stream);
    uint64_t segments = 0, passes = 0;
    int cur = 0;
    for (int pass = 0;; ++pass) {
        if (pass > 100000) return setError(PG_ERR_DEVICE, "%s: transmittance loop did not terminate", r.isectTr ? "pg_intersect_tr_at" : "pg_transmittance_at");
        uint64_t nk = 0;
        if (int e = queueSize(stream, q[cur].counts, nk)) return e;  // the pass's one wait
        if (nk == 0) break;
        launch_closest(dsc, s->trace, q[cur], (float4 *)s->tHit.p, (float *)s->tT.p, (TraceCounters *)s->traceCn.p, (int *)s->cursors.p, (int *)s->cullGuard.p, stream);
        segments += nk; ++passes;
        HIP_TRY(hipMemsetAsync(q[cur ^ 1].counts, 0, QSTRIDE * sizeof(int), stream));
        if (r.isect) launch_interaction(dsc, q[cur], (const float4 *)s->tHit.p, (const float *)s->tT.p, times[cur], (PgInteraction *)s->mqIsect.p, stream);
        launch_tr_step(dsc, r.isectTr, q[cur], times[cur], (const float4 *)s->tHit.p, (const float *)s->tT.p, state, r.u, r.nU, q[cur ^ 1], times[cur ^ 1], r.out,
                       (const PgInteraction *)s->mqIsect.p, r.isect, stream);
        cur ^= 1;
    }
    HIP_TRY(hipGetLastError());
    if (int e = stage.download()) return e;
    return finishQuery(s, stream, false, segments, passes);
}
// The three entry points' shared refusals: name, the scene, n, the rays, the media and the draws
static int mediumQueryArgs(const char *name, PgScene *s, int32_t n, const float *o, const float *d, const float *tmax, const int32_t *medium, const float *u,
                           int32_t nU, const void *out, const void *extra) {
    if (int e = checkArgs(name, s, n, {o, d, tmax, medium, out, extra})) return e;
    if (nU < 0 || (n > 0 && nU > 0 && !u)) return setError(PG_ERR_INVALID, "%s: n_u = %d %s", name, nU, nU < 0 ? "is negative" : "without a stream of draws: null argument");
    return PG_OK;
}
int pg_transmittance_at(PgScene *s, int32_t n, const float *o, const float *d, const float *tmax, const float *time, const float *p1, const int32_t *medium,
                        const float *u, int32_t nU, PgTransmittance *out, int mem, void *streamPtr) {
    if (int e = mediumQueryArgs("pg_transmittance_at", s, n, o, d, tmax, medium, u, nU, out, p1)) return e;
    if (n == 0) return PG_OK;
    const MediumQuery r = {n, o, d, tmax, time, p1, medium, u, nU, out, false, nullptr, nullptr, mem, streamPtr};
    return withExactFallback(s, [&]() { return mediumQuery(s, r); });
}
int pg_intersect_tr_at(PgScene *s, int32_t n, const float *o, const float *d, const float *tmax, const float *time, const int32_t *medium, const float *u,
                       int32_t nU, PgTransmittance *out, PgInteraction *isect, int mem, void *streamPtr) {
    if (int e = mediumQueryArgs("pg_intersect_tr_at", s, n, o, d, tmax, medium, u, nU, out, out)) return e;
    if (n == 0) return PG_OK;
    const MediumQuery r = {n, o, d, tmax, time, nullptr, medium, u, nU, out, true, isect, nullptr, mem, streamPtr};
    return withExactFallback(s, [&]() { return mediumQuery(s, r); });
}
int pg_medium_sample_at(PgScene *s, int32_t n, const float *o, const float *d, const float *tmax, const float *time, const int32_t *medium, const float *u,
                        int32_t nU, PgMediumSample *out, int mem, void *streamPtr) {
    if (int e = mediumQueryArgs("pg_medium_sample_at", s, n, o, d, tmax, medium, u, nU, out, out)) return e;
    if (n == 0) return PG_OK;
    return mediumQuery(s, {n, o, d, tmax, time, nullptr, medium, u, nU, nullptr, false, nullptr, out, mem, streamPtr});
}

// ---- batched BSSRDF::Sample_S at the rays' closest hits, and the BSDF it installs at the exit point ----
struct SubsurfaceQuery {
    int32_t n;
    const float *o, *d, *tmax, *time, *u;  // u: three floats per ray
    PgInteraction *po, *pi;  // po may be nullptr
    PgSubsurfaceSample *out;
    int mem;
    void *stream;
};
// packRays, one closest-hit launch as pg_intersect_at's (k_interaction into po where asked for), k_sss_seed, then sssProbeChains over this call's
// own queues -- the job queue and two probe queues of the test queue's geometry -- with the SssState indexed by ray number in grow-only scratch, and
// k_sss_emit.  The first walk's launches count (and k_sss_tally notes each probe ray for its sample's chain_rays).  One wait per step, for the number
// of chains still under way.
static int subsurfaceQuery(PgScene *s, SubsurfaceQuery r) {
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = (hipStream_t)r.stream;
    const size_t n = (size_t)r.n;
    const bool vol = s->nMedia > 0;
    Staging stage(s, r.mem, stream);
    stage.rays(r.o, r.d, r.tmax, r.time, n);
    stage.in(r.u, 3 * n);
    stage.out(r.out, n); stage.out(r.pi, n); stage.out(r.po, n);
    if (int e = stage.upload()) return e;
    RayQueue q;
    float *times = nullptr;
    if (int e = packRays(s, r.n, r.o, r.d, r.tmax, r.time, stream, q, times)) return e;
    const int cap = q.regionCap;
    const size_t N = (size_t)cap * PG_REGIONS;
    // (the records by queue entry: the probe queues are not filled front to back)
    DScene dsc = s->d;
    if (int e = queryScene(s, N, dsc)) return e;
    HIP_TRY(reserve(s->tHit, sizeof(float4) * N)); HIP_TRY(reserve(s->tT, sizeof(float) * N));
    // --- the job queue and the two probe queues, the state by ray
    RayQueue sq[3];
    float *probeTimes = nullptr;  // (k_sss_probe finds them behind d itself)
    HIP_TRY(reserve(s->ssCount, 3 * QSTRIDE * sizeof(int)));
    for (int k = 0; k < 3; ++k)
        if (int e = queueOver(s->ssO[k], s->ssD[k], (int *)s->ssCount.p + k * QSTRIDE, cap, sq[k], probeTimes)) return e;
    HIP_TRY(reserve(s->ssState, n * (10 * sizeof(float4) + 2 * sizeof(int2) + 2 * sizeof(int))));
    if (dsc.hasMotion) HIP_TRY(reserve(s->ssXf, (dsc.hasNest ? 2 : 1) * n * PG_XF_STRIDE * sizeof(float)));
    SssState st = {};
    float4 *f4 = (float4 *)s->ssState.p;
    st.po = f4; st.frame[0] = f4 + n; st.frame[1] = f4 + 2 * n; st.frame[2] = f4 + 3 * n; st.coef[0] = f4 + 4 * n; st.coef[1] = f4 + 5 * n;
    st.target = f4 + 6 * n; st.hit = f4 + 7 * n; st.hitO = f4 + 8 * n; st.hitD = f4 + 9 * n;
    st.count = (int2 *)(f4 + 10 * n); st.medium = st.count + n; st.hitInst = (int *)(st.medium + n);
    int *chain = st.hitInst + n;
    st.hitXf = dsc.hasMotion ? (float *)s->ssXf.p : nullptr; st.hitXfNest = r.n;
    st.qjob = sq[0];
    TraceCounters *cn = (TraceCounters *)s->traceCn.p;
    float4 *hits = (float4 *)s->tHit.p;
    launch_closest(dsc, s->trace, q, hits, (float *)s->tT.p, cn, (int *)s->cursors.p, (int *)s->cullGuard.p, stream);
    if (r.po) launch_interaction(dsc, q, hits, (const float *)s->tT.p, times, r.po, stream);
    HIP_TRY(hipMemsetAsync(st.qjob.counts, 0, QSTRIDE * sizeof(int), stream));
    launch_sss_seed(dsc, vol, q, hits, times, r.u, r.n, st, chain, r.out, r.pi, stream);
    uint64_t nJobs = 0, chainRays = 0, steps = 0;
    if (int e = queueSize(stream, st.qjob.counts, nJobs)) return e;
    if (int e = sssProbeChains("pg_subsurface_sample_at", s, dsc, st, sq + 1, hits, cn, nJobs, vol, stream,
                               [&](const RayQueue &curQ, uint64_t nRays) { chainRays += nRays; ++steps; launch_sss_tally(curQ, chain, stream); })) return e;
    if (nJobs > 0) launch_sss_emit(dsc, vol, st, chain, times, r.out, r.pi, stream);
    HIP_TRY(hipGetLastError());
    if (int e = stage.download()) return e;
    return finishQuery(s, stream, false, n + chainRays, 1 + steps);
}
int pg_subsurface_sample_at(PgScene *s, int32_t n, const float *o, const float *d, const float *tmax, const float *time, const float *u, PgInteraction *po,
                            PgInteraction *pi, PgSubsurfaceSample *out, int mem, void *streamPtr) {
    if (int e = checkArgs("pg_subsurface_sample_at", s, n, {o, d, tmax, u, pi, out})) return e;
    if (n == 0) return PG_OK;
    const SubsurfaceQuery r = {n, o, d, tmax, time, u, po, pi, out, mem, streamPtr};
    return withExactFallback(s, [&]() { return subsurfaceQuery(s, r); });
}
// The two exit-BSDF calls: stage, k_adapter, copy back, one wait.  Nothing is traced and no counter moves.
static int adapterQuery(const char *name, PgScene *s, int32_t n, const PgInteraction *pi, const float *eta, const float *in, bool sample, int32_t flags,
                        PgScatter *out, int mem, void *streamPtr) {
    if (int e = checkArgs(name, s, n, {pi, eta, in, out}, flags)) return e;
    if (n == 0) return PG_OK;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t stream = (hipStream_t)streamPtr;
    const size_t nn = (size_t)n;
    Staging stage(s, mem, stream);
    stage.in(pi, nn); stage.in(eta, nn); stage.in(in, (sample ? 2 : 3) * nn);
    stage.out(out, nn);
    if (int e = stage.upload()) return e;
    launch_adapter(pi, eta, in, sample, flags, n, out, stream);
    HIP_TRY(hipGetLastError());
    if (int e = stage.download()) return e;
    HIP_TRY(hipStreamSynchronize(stream));
    return PG_OK;
}
int pg_subsurface_f_at(PgScene *s, int32_t n, const PgInteraction *pi, const float *eta, const float *wi, int32_t flags, PgScatter *out, int mem, void *streamPtr) {
    return adapterQuery("pg_subsurface_f_at", s, n, pi, eta, wi, false, flags, out, mem, streamPtr);
}
int pg_subsurface_sample_f_at(PgScene *s, int32_t n, const PgInteraction *pi, const float *eta, const float *u, int32_t flags, PgScatter *out, int mem,
                              void *streamPtr) {
    return adapterQuery("pg_subsurface_sample_f_at", s, n, pi, eta, u, true, flags, out, mem, streamPtr);
}

int pg_counters(PgScene *s, PgCounters *out) {
    if (!s || !out) return setError(PG_ERR_INVALID, "pg_counters: null argument");
    memcpy(out, &s->counters, s->callerAbi >= 30 ? sizeof(PgCounters) : PG_ABI29_COUNTERS_BYTES);
    return PG_OK;
}
int pg_scene_set_option(PgScene *s, int32_t option, int32_t value) {
    if (!s) return setError(PG_ERR_INVALID, "pg_scene_set_option: null scene");
    switch (option) {
    case PG_OPT_OVERLAP_SHADOW: s->overlapShadow = value != 0; return PG_OK;
    default: return setError(PG_ERR_INVALID, "pg_scene_set_option: unknown option %d", option);
    }
}
int pg_counters_reset(PgScene *s) {
    if (!s) return setError(PG_ERR_INVALID, "pg_counters_reset: null argument");
    HIP_TRY(hipSetDevice(s->device));
    memset(&s->counters, 0, sizeof(s->counters));
    HIP_TRY(hipMemset(s->traceCn.p, 0, s->traceCn.bytes));
    HIP_TRY(hipMemset(s->lightTests.p, 0, s->lightTests.bytes));
    return PG_OK;
}
}  // extern "C"
