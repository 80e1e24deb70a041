// Camera "realistic": the host half of cameras/realistic.cpp -- the lens file, the constructor's focusing and the 64 exit pupil boxes.  The
// lens arithmetic itself (TraceLensesFromFilm and friends) is csrc/pg_lens.h, shared with the device, which traces every camera sample.
//   CreateRealisticCamera            realistic.cpp:714-752, floatfile.cpp:40-82
//   RealisticCamera::RealisticCamera :50-98
//   ComputeThickLensApproximation / FocusThickLens / FocusBinarySearch / FocusDistance   :429-531
//   BoundExitPupil                   :534-571
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <thread>
#include <vector>
#include "api.h"
#include "error.h"
#include "scene.h"

namespace pbrt {
namespace {

// ReadFloatFile, floatfile.cpp:40-82: '#' comments, numbers separated by anything that is not part of one (a number that runs into the end
// of the file without a separator is not stored, as there)
bool ReadFloatFile(const char *filename, std::vector<Float> *values) {
    FILE *f = fopen(filename, "r");
    if (!f) {
        Error("Unable to open file \"%s\"", filename);
        return false;
    }
    int c;
    bool inNumber = false;
    char curNumber[32];
    int curNumberPos = 0, lineNumber = 1;
    while ((c = getc(f)) != EOF) {
        if (c == '\n') ++lineNumber;
        if (inNumber) {
            if (curNumberPos >= (int)sizeof(curNumber)) {  // (the reference's CHECK_LT ends its process here)
                Error("Overflowed buffer for parsing number in file: %s, at line %d", filename, lineNumber);
                fclose(f);
                return false;
            }
            if (isdigit(c) || c == '.' || c == 'e' || c == '-' || c == '+') curNumber[curNumberPos++] = (char)c;
            else {
                curNumber[curNumberPos++] = '\0';
                values->push_back((Float)atof(curNumber));
                inNumber = false;
                curNumberPos = 0;
            }
        } else {
            if (isdigit(c) || c == '.' || c == '-' || c == '+') {
                inNumber = true;
                curNumber[curNumberPos++] = (char)c;
            } else if (c == '#') {
                while ((c = getc(f)) != '\n' && c != EOF)
                    ;
                ++lineNumber;
            } else if (!isspace(c))
                Warning("Unexpected text found at line %d of float file \"%s\"", lineNumber, filename);
        }
    }
    fclose(f);
    return true;
}

// RadicalInverse(0, a) and RadicalInverse(1, a), lowdiscrepancy.cpp:389-403 / lowdiscrepancy.h:76-79
Float RadicalInverse2(uint64_t a) {
    uint64_t r = 0;
    for (int i = 0; i < 64 && a; ++i, a >>= 1) if (a & 1) r |= (uint64_t)1 << (63 - i);
    return (Float)((double)r * 5.4210108624275222e-20);  // 0x1p-64
}
Float RadicalInverse3(uint64_t a) {
    const Float invBase = (Float)1 / (Float)3;
    uint64_t reversedDigits = 0;
    Float invBaseN = 1;
    while (a) {
        const uint64_t next = a / 3, digit = a - next * 3;
        reversedDigits = reversedDigits * 3 + digit;
        invBaseN *= invBase;
        a = next;
    }
    return std::min(reversedDigits * invBaseN, 0.99999994f);  // OneMinusEpsilon
}

struct Bounds2 { Float x0, y0, x1, y1; };
int LensThreads() {  // never the whole machine: the pool serves 64 + a few calls of a second each
    int nt = PbrtOptions.nThreads > 0 ? PbrtOptions.nThreads : (int)std::thread::hardware_concurrency();
    return std::max(1, std::min(nt, 16));
}
// RealisticCamera::BoundExitPupil, realistic.cpp:534-571.  A sample that lies inside the bounds so far, or whose ray does not leave the lens,
// never changes the bounds: the result is the box of all samples whose ray leaves the lens, whatever the order -- so each thread keeps the box
// of its own share (with the same shortcut) and the boxes are merged by min / max.
Bounds2 BoundExitPupil(const PgLensSystem &L, Float pFilmX0, Float pFilmX1) {
    const int nSamples = 1024 * 1024;
    const Float rearRadius = L.iface[L.n - 1][3];  // RearElementRadius
    const Bounds2 proj = {-1.5f * rearRadius, -1.5f * rearRadius, 1.5f * rearRadius, 1.5f * rearRadius};
    const Float rearZ = lens_rear_z(L);
    const int nt = LensThreads();
    const Float big = std::numeric_limits<Float>::max(), low = std::numeric_limits<Float>::lowest();
    std::vector<Bounds2> part((size_t)nt, Bounds2{big, big, low, low});  // Bounds2(): pMin = max, pMax = lowest (geometry.h:568-573)
    std::vector<int> exiting((size_t)nt, 0);
    auto work = [&](int t) {
        Bounds2 b = part[(size_t)t];
        int n = 0;
        for (int i = nSamples / nt * t, end = t == nt - 1 ? nSamples : nSamples / nt * (t + 1); i < end; ++i) {
            const Float pFilmX = lens_lerp((i + 0.5f) / nSamples, pFilmX0, pFilmX1);
            const Float u0 = RadicalInverse2((uint64_t)i), u1 = RadicalInverse3((uint64_t)i);
            const Float rx = lens_lerp(u0, proj.x0, proj.x1), ry = lens_lerp(u1, proj.y0, proj.y1);
            bool through = rx >= b.x0 && rx <= b.x1 && ry >= b.y0 && ry <= b.y1;  // Inside(pRear, pupilBounds)
            if (!through) {
                LensRay r;
                r.o = lens_v(pFilmX, 0, 0);
                r.d = lens_sub(lens_v(rx, ry, rearZ), r.o);
                through = lens_trace_from_film(L, r, nullptr);
            }
            if (through) {
                b.x0 = std::min(b.x0, rx); b.y0 = std::min(b.y0, ry); b.x1 = std::max(b.x1, rx); b.y1 = std::max(b.y1, ry);
                ++n;
            }
        }
        part[(size_t)t] = b; exiting[(size_t)t] = n;
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) pool.emplace_back(work, t);
    work(0);
    for (auto &th : pool) th.join();
    Bounds2 b = part[0];
    int nExitingRays = exiting[0];
    for (int t = 1; t < nt; ++t) {
        b.x0 = std::min(b.x0, part[(size_t)t].x0); b.y0 = std::min(b.y0, part[(size_t)t].y0);
        b.x1 = std::max(b.x1, part[(size_t)t].x1); b.y1 = std::max(b.y1, part[(size_t)t].y1);
        nExitingRays += exiting[(size_t)t];
    }
    if (nExitingRays == 0) return proj;  // the whole projected rear element
    // Expand(pupilBounds, 2 * projRearBounds.Diagonal().Length() / std::sqrt(nSamples)): a float over a double, rounded to Float by Vector2f(delta, delta)
    const Float dx = proj.x1 - proj.x0, dy = proj.y1 - proj.y0;
    const Float delta = (Float)((double)(2 * std::sqrt(dx * dx + dy * dy)) / std::sqrt((double)nSamples));
    return Bounds2{b.x0 - delta, b.y0 - delta, b.x1 + delta, b.y1 + delta};
}

// ComputeCardinalPoints, realistic.cpp:429-435
void ComputeCardinalPoints(const LensRay &rIn, const LensRay &rOut, Float *pz, Float *fz) {
    const Float tf = -rOut.o.x / rOut.d.x;
    *fz = -(rOut.o.z + rOut.d.z * tf);
    const Float tp = (rIn.o.x - rOut.o.x) / rOut.d.x;
    *pz = -(rOut.o.z + rOut.d.z * tp);
}
// FocusThickLens, realistic.cpp:437-472.  false: one of the reference's CHECKs (:445, :452, :468) would have ended its process -- an Error
// has been reported and the frame must be refused.
bool FocusThickLens(const PgLensSystem &L, Float focusDistance, Float *thickness) {
    Float pz[2], fz[2];
    const Float x = (Float)(.001 * (double)L.diagonal);
    LensRay rScene, rFilm;
    rScene.o = lens_v(x, 0, lens_front_z(L) + 1); rScene.d = lens_v(0, 0, -1);
    bool negativeT = false;
    if (!lens_trace_from_scene(L, rScene, &rFilm, &negativeT)) {
        Error("Unable to trace ray from scene to film for thick lens approximation. Is aperture stop extremely small?");
        return false;
    }
    ComputeCardinalPoints(rScene, rFilm, &pz[0], &fz[0]);
    rFilm.o = lens_v(x, 0, lens_rear_z(L) - 1); rFilm.d = lens_v(0, 0, 1);
    if (!lens_trace_from_film(L, rFilm, &rScene)) {
        Error("Unable to trace ray from film to scene for thick lens approximation. Is aperture stop extremely small?");
        return false;
    }
    ComputeCardinalPoints(rFilm, rScene, &pz[1], &fz[1]);
    const Float f = fz[0] - pz[0];
    const Float z = -focusDistance;
    const Float c = (pz[1] - z - pz[0]) * (pz[1] - z - 4 * f - pz[0]);
    if (!(c > 0)) {
        Error("Coefficient must be positive. It looks focusDistance: %f is too short for a given lenses configuration", focusDistance);
        return false;
    }
    const Float delta = 0.5f * (pz[1] - z + pz[0] - std::sqrt(c));
    *thickness = lens_rear_z(L) + delta;
    return true;
}
// FocusDistance, realistic.cpp:495-531.  `bounds` = BoundExitPupil(0, .001 * film->diagonal): the lens does not change while the binary
// search runs, so the search computes the box once.
Float FocusDistance(const PgLensSystem &L, const Bounds2 &bounds, Float filmDistance) {
    const Float scaleFactors[3] = {0.1f, 0.01f, 0.001f};
    Float lu = 0.0f;
    LensRay ray;
    bool foundFocusRay = false;
    for (Float scale : scaleFactors) {
        lu = scale * bounds.x1;
        LensRay r;
        r.o = lens_v(0, 0, lens_rear_z(L) - filmDistance); r.d = lens_v(lu, 0, filmDistance);
        if (lens_trace_from_film(L, r, &ray)) { foundFocusRay = true; break; }
    }
    if (!foundFocusRay) {
        Error("Focus ray at lens pos(%f,0) didn't make it through the lenses with film distance %f?!??\n", lu, filmDistance);
        return Infinity;
    }
    const Float tFocus = -ray.o.x / ray.d.x;
    Float zFocus = ray.o.z + ray.d.z * tFocus;
    if (zFocus < 0) zFocus = Infinity;
    return zFocus;
}
// FocusBinarySearch, realistic.cpp:474-493.  Its result is only logged by the constructor (:75-77), but it can report FocusDistance's Error, so
// it runs.  (A film distance that has left the finite floats ends the two widening loops, which the reference would spin in for ever.)
Float FocusBinarySearch(const PgLensSystem &L, Float focusDistance, Float thickLens) {
    const Bounds2 bounds = BoundExitPupil(L, 0, (Float)(.001 * (double)L.diagonal));
    Float filmDistanceLower = thickLens, filmDistanceUpper = thickLens;
    while (FocusDistance(L, bounds, filmDistanceLower) > focusDistance && std::isfinite(filmDistanceLower)) filmDistanceLower *= 1.005f;
    while (FocusDistance(L, bounds, filmDistanceUpper) < focusDistance && filmDistanceUpper != 0 && std::isfinite(filmDistanceUpper)) filmDistanceUpper /= 1.005f;
    for (int i = 0; i < 20; ++i) {
        const Float fmid = 0.5f * (filmDistanceLower + filmDistanceUpper);
        const Float midFocus = FocusDistance(L, bounds, fmid);
        if (midFocus < focusDistance) filmDistanceLower = fmid;
        else filmDistanceUpper = fmid;
    }
    return 0.5f * (filmDistanceLower + filmDistanceUpper);
}
}  // namespace

PerspectiveCamera *CreateRealisticCamera(const ParamSet &params, const Transform &cam2world, Film *film, bool *refused) {
    Float shutteropen = params.FindOneFloat("shutteropen", 0.f);
    Float shutterclose = params.FindOneFloat("shutterclose", 1.f);
    if (shutterclose < shutteropen) {
        Warning("Shutter close time [%f] < shutter open [%f].  Swapping them.", shutterclose, shutteropen);
        std::swap(shutterclose, shutteropen);
    }
    std::string lensFile = params.FindOneString("lensfile", "");  // FindOneFilename, paramset.cpp
    if (lensFile != "") lensFile = AbsolutePath(ResolveFilename(lensFile));
    const Float apertureDiameter = params.FindOneFloat("aperturediameter", 1.0);
    const Float focusDistance = params.FindOneFloat("focusdistance", 10.0);
    const bool simpleWeighting = params.FindOneBool("simpleweighting", true);
    if (lensFile == "") {
        Error("No lens description file supplied!");
        return nullptr;
    }
    std::vector<Float> lensData;
    if (!ReadFloatFile(lensFile.c_str(), &lensData)) {
        Error("Error reading lens specification file \"%s\".", lensFile.c_str());
        return nullptr;
    }
    if (lensData.size() % 4 != 0) {
        Error("Excess values in lens specification file \"%s\"; must be multiple-of-four values, read %d.", lensFile.c_str(), (int)lensData.size());
        return nullptr;
    }
    if (lensData.empty() || lensData.size() / 4 > PG_MAX_LENS_INTERFACES) {
        Error("Lens specification file \"%s\" has %d interfaces; this build traces 1 .. %d.", lensFile.c_str(), (int)(lensData.size() / 4), PG_MAX_LENS_INTERFACES);
        *refused = true;
        return nullptr;
    }
    // RealisticCamera::RealisticCamera, realistic.cpp:58-72
    PgLensSystem L = {};
    L.n = (int)(lensData.size() / 4);
    for (int i = 0; i < (int)lensData.size(); i += 4) {
        if (lensData[i] == 0) {
            if (apertureDiameter > lensData[i + 3])
                Warning("Specified aperture diameter %f is greater than maximum possible %f.  Clamping it.", apertureDiameter, lensData[i + 3]);
            else lensData[i + 3] = apertureDiameter;
        }
        float *e = L.iface[i / 4];
        e[0] = lensData[i] * (Float).001; e[1] = lensData[i + 1] * (Float).001; e[2] = lensData[i + 2]; e[3] = lensData[i + 3] * Float(.001) / Float(2.);
    }
    L.diagonal = film->diagonal;
    L.simple = simpleWeighting ? 1 : 0;
    film->GetPhysicalExtent(L.extent);
    // :74-81: the binary search's result is logged only; the thick lens approximation sets the film distance
    Float thick;
    // (FocusThickLens runs as FocusBinarySearch's first statement, :477, and again at :78 on the same lens: one call serves both)
    if (!FocusThickLens(L, focusDistance, &thick)) { *refused = true; return nullptr; }
    FocusBinarySearch(L, focusDistance, thick);
    L.iface[L.n - 1][1] = thick;
    // :83-90
    const int nSamples = PG_LENS_PUPIL_SEGMENTS;
    for (int i = 0; i < nSamples; ++i) {
        const Float r0 = (Float)i / nSamples * film->diagonal / 2;
        const Float r1 = (Float)(i + 1) / nSamples * film->diagonal / 2;
        const Bounds2 b = BoundExitPupil(L, r0, r1);
        L.pupil[i][0] = b.x0; L.pupil[i][1] = b.y0; L.pupil[i][2] = b.x1; L.pupil[i][3] = b.y1;
    }
    if (simpleWeighting)
        Warning("\"simpleweighting\" option with RealisticCamera no longer necessarily matches regular camera images. Further, pixel values will vary a bit "
                "depending on the aperture size. See this discussion for details: https://github.com/mmp/pbrt-v3/issues/162#issuecomment-348625837");
    PerspectiveCamera *cam = new PerspectiveCamera;
    cam->realistic = true;
    cam->lens = L;
    cam->film.reset(film);
    cam->CameraToWorld = cam2world;
    cam->lensRadius = 0; cam->focalDistance = 0;
    cam->shutterOpen = shutteropen; cam->shutterClose = shutterclose;
    return cam;
}
}  // namespace pbrt
