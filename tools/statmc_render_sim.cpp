// statmc_render_sim -- the render loop of StatPathIntegrator::Render<T> (src/statistics/statpath.cpp:
// 120-445) around statmc::Estimator, with the path tracer replaced by a counter-based synthetic
// sample source.  It exercises the accumulation side of the drop-in exactly the way the reference
// drives it:
//
//   * 16 x 16 tiles (statpath.cpp:132), one set of StatTile<T> per tile from Estimator::GetTiles
//     (statpath.cpp:173-190), worker threads taking tiles (ParallelFor2D);
//   * per pixel and sample the Add*Sample* method selected from the stat type's configuration is
//     called through a member-function pointer (GetAddSampleFn, statpath.cpp:97-116, 355-371);
//   * Merge[Transform]Tiles once per tile and iteration from the worker thread (statpath.cpp:381-388);
//   * the exponential iteration schedule spp, spp, 2 spp, 4 spp, ... (statpath.cpp:272-279);
//   * Upload / Denoise / Download / Synchronize on the main thread, timed and printed like the
//     reference's "CUDA time [ns]" bracket (statpath.cpp:397-417);
//   * dumps named <stem>-<total spp>-<buffer>.pfm (OutputBufferSelection::Write, statpath.cpp:421-427).
//
// The tiles record samples; the moments are accumulated on the device (statmc_accumulate_tiles).
// The sample source is a pure function of (seed, x, y, sample index), restated in
// tests/test_render_sim_gpu.py so that the dumps can be checked against the CPU oracle.
//
//   statmc_render_sim --width 96 --height 56 --spp 4 --iterations 3 --stem out/sim [--threads 4]
//                     [--seed 1] [--filtersd 10] [--filterradius 20] [--stage-mb 2048] [--no-denoise]
//                     [--config denoise|acrr|smis] [--trackedbounces 5] [--outputregex '.*'] [--warmup] [--tilestats]
//                     [--adaptive] [--adaptive-pixels [--stop-at Q:T] [--stop-mean mean|rms:T[:CAP]] [--stop-tiles T:TOL[:CAP] [--tile-quantile NUM/DEN] [--close-tiles]] [--stop-metric sd|stderr|ci] [--target-error T]
//                     [--score-dilate R]]
//                     [--placed] [--half-features]
// --adaptive: per-tile sample budgets from the tile-local noise level (Estimator::TileNoise); see RenderLoop.
// --adaptive-pixels: per-pixel sample budgets planned on the device (Estimator::PlanSamples); see RenderLoop.
// --stop-at Q:T: with --adaptive-pixels, the stopping rule: after every iteration the Q-quantile (nearest rank) of the relative radiance
//                   score is selected on the device (Estimator::ScoreSelect); once it is <= T the remaining iterations are skipped.
// --stop-mean mean|rms:T[:CAP]: with --adaptive-pixels, a mean rule: after every iteration the exact sums of the relative radiance
//                   score are formed on the device (Estimator::ScoreSum), every pixel counting as min(score, CAP); once their mean
//                   (sum / n) or RMS (sqrt(sum of squares / n)) is <= T the remaining iterations are skipped.  CAP defaults to +inf:
//                   no cap, and the pixels nobody can judge yet (+inf) are left out of the sums and of n.  Reads --stop-metric's
//                   quantity and --score-dilate's window as --stop-at does; with --stop-at as well, both rules must hold.  Every
//                   iteration prints a "Mean rule:" line.  Not with --preview, for --stop-at's reason.
// --stop-tiles T:TOL[:CAP]: with --adaptive-pixels, a rule per region: after every iteration the relative radiance score's exact mean
//                   under CAP is formed per T x T tile on the device (T = 8, 16, 32 or 64; Estimator::ScoreTiles), and the tiles whose
//                   mean is above TOL -- the open tiles -- are counted on the tile grid (statmc_score_count_above on the mean plane):
//                   one int64 comes back.  Once no tile is open the remaining iterations are skipped.  CAP defaults to +inf.  Reads
//                   --stop-metric's quantity and --score-dilate's window; with --stop-at or --stop-mean as well, every rule must
//                   hold.  Every iteration prints a "Tile rule:" line with "open tiles k / N".  Not with --preview.
// --tile-quantile NUM/DEN: with --stop-tiles, the tile's statistic is the NUM/DEN-quantile of its pixels' scores by the nearest-rank rule
//                   (Estimator::ScoreTileQuantiles, 0 <= NUM <= DEN <= 65536) instead of their mean; CAP is not used.  The "Tile rule:" line
//                   says "quantile NUM/DEN of the relative ..." then.
// --close-tiles:    with --stop-tiles, a tile that has met the rule is closed for good: after every iteration the rule's plane goes through
//                   Estimator::GateTiles with a closed plane kept over the run; the next plan's score is gated, its budget is the schedule's
//                   samples per pixel times the open pixels, its lower bound 0, and the planned counts are gated again (Estimator::PlanSamples
//                   with a TileGate).  The run ends when no tile is open.  Every iteration prints "Closed tiles: iteration i, closed now A,
//                   open B / N, open pixels P".  A render tile whose pixels all have a count of 0 is skipped: no sample is added and its
//                   Merge*Tile(s) calls are not made.  Not with --target-error.
// --stop-metric M: which quantity --stop-at's quantile (and --target-error's plan) reads.  sd, the default: the sample standard
//                   deviation, which does not fall as samples arrive -- only T = 0 or a T above the film's noise make sense with it;
//                   stderr: the standard error of the mean; ci: the two-sided confidence half-width at the device's significance
//                   level (Estimator's scoreOf).  With stderr or ci every iteration prints a "Stop metric:" line with the quantile.
// --target-error T: with --adaptive-pixels, the next iteration's counts are the samples that bring every pixel's relative error
//                   (--stop-metric's; ci if that is sd) to T, 1 .. 4 * target per pixel (Estimator::PlanToTarget), under the schedule's
//                   budget: a plan that asks for more falls back to the budget plan.  Prints "Planned to target:".
// --score-dilate R: with --adaptive-pixels, the plan and --stop-at's quantile read the worst score within R pixels (0 to 32) of every
//                   pixel instead of the pixel's own (statmc_score_window, MAX: Estimator::PlanSamples' / ScoreSelect's scoreDilate).
// --half-features: every stat type without the radiance transform (normal, albedo, the MIS tallies) is staged and uploaded in IEEE
//                   half (Estimator::SetSampleFormat); radiance stays fp32.  "Staged bytes:" at the end counts what went up.
// --preview K: every iteration but the last denoises through the preview path -- the film pooled K x K (2, 4 or 8), that coarse film
//                   denoised, its result brought back onto the fine film (Estimator::DenoisePreview, statmc_upsample_filtered) --, the last
//                   through the full filter.  The dumps and the timing lines keep their form.  Not with --stop-at: which iteration is the
//                   last is then not known before its denoise pass.
// --config denoise: Render<Vec3>, RGB radiance + normal + albedo, filter<float3> (scenes/render-denoise.pbrt).
// --config acrr:    Render<Float>, "multichannelstats" false: the luminance of the path prefix up to each
//                   of the tracked bounces is one float stat buffer, filtered together by filter<float>
//                   (scenes/acrr.pbrt; estimator.cpp:434-460).
// --config smis:    no radiance statistics; per tracked bounce two float tallies (BSDF / light win rate,
//                   plain M3) through the nested MergeTiles overload, filter<float> over 2 x bounces buffers.
//   statmc_render_sim [--seed 1] --print-sample x y s     (prints one generated sample, no device)
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <thread>

#include "statmc_denoiser.hpp"
#include "statmc_pfm.hpp"

using namespace statmc;

// ---- synthetic sample source (all arithmetic in fp32, one rounding per operation) --------------
static inline uint32_t mix(uint32_t a) {  // lowbias32
    a ^= a >> 16;
    a *= 0x7feb352dU;
    a ^= a >> 15;
    a *= 0x846ca68bU;
    a ^= a >> 16;
    return a;
}
static inline uint32_t draw(uint32_t seed, int x, int y, uint32_t sample, uint32_t stream) {
    return mix(mix(mix(seed ^ (0x9e3779b9U * (uint32_t)(x + 65536 * y))) + sample) + stream * 0x85ebca6bU);
}
static inline float unit(uint32_t key) { return (float)(key >> 8) * (1.0f / 16777216.0f); }

static const float kAlbedo[3][3] = {{0.80f, 0.25f, 0.20f}, {0.15f, 0.55f, 0.85f}, {0.60f, 0.60f, 0.10f}};
static const float kNormal[3][3] = {{0.0f, 0.0f, 1.0f}, {0.6f, -0.8f, 0.0f}, {-0.7071f, 0.0f, 0.7071f}};

struct PixelSample {
    Vec3 radiance, normal, albedo;
};
// GetStatSample<T> (statpath.h): the RGB triple, or its luminance (RGBSpectrum::y(), spectrum.h)
template <typename T>
static T GetStatSample(const Vec3 &L);
template <>
Vec3 GetStatSample<Vec3>(const Vec3 &L) { return L; }
template <>
float GetStatSample<float>(const Vec3 &L) { return 0.212671f * L.x + 0.715160f * L.y + 0.072169f * L.z; }
static PixelSample makeSample(uint32_t seed, int x, int y, uint32_t s) {
    const int region = ((x / 24) + (y / 20)) % 3;
    const float e = 0.5f + 0.5f * ((float)((x * 7 + y * 3) % 32) / 32.0f);
    const bool black = (draw(seed, x, y, s, 3) & 7u) == 0u;  // zero-radiance paths
    float rad[3], nrm[3], alb[3];
    for (int c = 0; c < 3; c++) {
        const float u = unit(draw(seed, x, y, s, (uint32_t)c));
        const float t = 4.0f * (u * u);
        rad[c] = black ? 0.0f : (kAlbedo[region][c] * e) * t;
        nrm[c] = kNormal[region][c] + (unit(draw(seed, x, y, s, 4u + c)) - 0.5f) * 0.02f;
        alb[c] = kAlbedo[region][c] + (unit(draw(seed, x, y, s, 7u + c)) - 0.5f) * 0.01f;
    }
    return PixelSample{Vec3{rad[0], rad[1], rad[2]}, Vec3{nrm[0], nrm[1], nrm[2]}, Vec3{alb[0], alb[1], alb[2]}};
}

// GetAddSampleFn (statpath.cpp:97-116)
template <typename T>
using AddSampleFn = void (StatTile<T>::*)(const Point2i, const T);
template <typename T>
static AddSampleFn<T> GetAddSampleFn(const StatTypeConfig &cfg) {
    if (cfg.transform) {
        if (cfg.maxMoment == 3) return &StatTile<T>::AddTransformSampleM3;
        if (cfg.maxMoment == 2) return &StatTile<T>::AddTransformSampleM2;
        if (cfg.maxMoment == 1) return &StatTile<T>::AddTransformSampleM1;
    } else {
        if (cfg.maxMoment == 3) return &StatTile<T>::AddSampleM3;
        if (cfg.maxMoment == 2) return &StatTile<T>::AddSampleM2;
        if (cfg.maxMoment == 1) return &StatTile<T>::AddSampleM1;
    }
    return nullptr;
}

struct Options {
    int width = 96, height = 56, spp = 4, iterations = 3, threads = 4, stageMb = 2048, trackedBounces = 5;
    unsigned seed = 1;
    float filterSD = 10.f;
    int filterRadius = 20;
    bool denoise = true, acrr = false, smis = false, warmUp = false, tileStats = false, adaptive = false, adaptivePixels = false, halfFeatures = false;
    bool stopAt = false;       // --stop-at Q:T
    double stopQuantile = 0.0;
    float stopThreshold = 0.f;
    bool stopMean = false;     // --stop-mean mean|rms:T[:CAP]
    bool stopMeanRms = false;
    float stopMeanTarget = 0.f, stopMeanCap = INFINITY;
    bool stopTiles = false;    // --stop-tiles T:TOL[:CAP]
    int stopTilesTile = 0;
    float stopTilesTol = 0.f, stopTilesCap = INFINITY;
    bool tileQuantile = false, closeTiles = false;   // --tile-quantile NUM/DEN, --close-tiles
    int tileQuantileNum = 0, tileQuantileDen = 1;
    int stopMetric = Estimator::ScoreOfDeviation;   // --stop-metric sd|stderr|ci
    bool stopMetricGiven = false;
    bool targetErrorGiven = false;   // --target-error T
    float targetError = 0.f;
    bool scoreDilateGiven = false;   // --score-dilate R
    int scoreDilate = 0;
    int preview = 0;           // --preview K
    std::string stem, outputRegex = ".*";
};

template <typename T>
static void Render(const Options &o) {
    const int width = o.width, height = o.height;
    StatPathParams params;
    params.acrr = o.acrr;
    params.smis = o.smis;
    params.multiChannelStats = !o.acrr;
    params.trackedBounces = o.trackedBounces;
    params.denoiseImage = o.denoise && !o.acrr && !o.smis;
    params.calcStats = !o.denoise && !o.acrr && !o.smis;
    params.filterSD = o.filterSD;
    params.filterRadius = (unsigned char)o.filterRadius;
    const StatTypeConfigs sCfgs = makeStatTypeConfigs(params);
    // `film` itself is not denoised here (no Film in this harness): the colour images are the
    // t0-b<j>-film-mean buffers, the results t0-b<j>-film-mean-f.
    Buffer film("film", HostImage(height, width, F32C3));
    BufferRegistry reg(film);
    Estimator estimator(film, sCfgs, o.filterSD, (unsigned char)o.filterRadius, /*denoiseFilm=*/false, o.acrr, o.smis, reg);
    estimator.AllocateBuffers(reg);
    if (o.halfFeatures)
        for (unsigned char t = 0; t < estimator.statTypeConfigs.nEnabled; t++)
            if (!estimator.statTypeConfigs.configs[t].transform) estimator.SetSampleFormat(t, STATMC_SAMPLES_F16);
    estimator.EnableDeviceAccumulation((size_t)o.stageMb << 20);
    // --preview: the coarse film, an Estimator of the same configuration that nothing accumulates into
    std::unique_ptr<Buffer> coarseFilm;
    std::unique_ptr<BufferRegistry> coarseReg;
    std::unique_ptr<Estimator> coarseEst;
    if (o.preview) {
        const int wc = (width + o.preview - 1) / o.preview, hc = (height + o.preview - 1) / o.preview;
        coarseFilm.reset(new Buffer("film", HostImage(hc, wc, F32C3)));
        coarseReg.reset(new BufferRegistry(*coarseFilm));
        coarseEst.reset(new Estimator(*coarseFilm, sCfgs, o.filterSD, (unsigned char)o.filterRadius, /*denoiseFilm=*/false, o.acrr, o.smis, *coarseReg));
        coarseEst->AllocateBuffers(*coarseReg);
        coarseEst->SetPipelineBands(1);
    }

    std::vector<StatTypeConfig> enabledRGBFeatureCfgs;  // statpath.cpp:160-163
    for (unsigned char t : {(unsigned char)StatMaterialID, (unsigned char)StatDepth, (unsigned char)StatNormal,
                            (unsigned char)StatAlbedo})
        if (sCfgs[t].enable && sCfgs[t].nChannels == 3) enabledRGBFeatureCfgs.push_back(sCfgs[t]);
    const unsigned char nRGBBuffers = (unsigned char)enabledRGBFeatureCfgs.size();
    if (nRGBBuffers != 2) throw std::runtime_error("expected the normal and albedo feature types");

    AddSampleFn<T> AddLSampleFn = GetAddSampleFn<T>(sCfgs[Radiance]);
    AddSampleFn<float> AddMISWinRateSampleFn = GetAddSampleFn<float>(sCfgs[MISBSDFWinRate]);
    AddSampleFn<Vec3> AddRGBGBufferSampleFn = GetAddSampleFn<Vec3>(sCfgs[StatNormal]);
    const bool misEnabled = sCfgs[MISBSDFWinRate].enable && sCfgs[MISLightWinRate].enable;
    const std::vector<StatTypeConfig> misCfgs = {sCfgs[MISBSDFWinRate], sCfgs[MISLightWinRate]};
    const unsigned char nLs = sCfgs[Radiance].bounceEnd;

    const int tileSize = 16;  // statpath.cpp:132
    const int nTilesX = (width + tileSize - 1) / tileSize, nTilesY = (height + tileSize - 1) / tileSize;
    const int nTilesTotal = nTilesX * nTilesY;
    std::vector<std::vector<StatTile<T>>> lTiles(nTilesTotal);
    std::vector<std::vector<std::vector<StatTile<Vec3>>>> rgbFeatureTiles(nTilesTotal);
    std::vector<std::vector<std::vector<StatTile<float>>>> misTallyTiles(nTilesTotal);
    auto tileBoundsOf = [&](int tileIndex) {
        const int tx = tileIndex % nTilesX, ty = tileIndex / nTilesX;
        return Bounds2i(Point2i(tx * tileSize, ty * tileSize),
                        Point2i(std::min((tx + 1) * tileSize, width), std::min((ty + 1) * tileSize, height)));
    };
    for (int t = 0; t < nTilesTotal; t++) {  // statpath.cpp:173-190
        lTiles[t] = estimator.GetTiles<T>(tileBoundsOf(t), sCfgs[Radiance].bounceEnd);
        rgbFeatureTiles[t] = estimator.GetTiles<Vec3>(tileBoundsOf(t), 1, nRGBBuffers);
        misTallyTiles[t] = estimator.GetTiles<float>(tileBoundsOf(t), sCfgs[MISBSDFWinRate].bounceEnd, 2);
    }

    const OutputBufferSelection outBufSel(reg, std::regex(o.outputRegex), (o.stem.empty() ? std::string("out") : o.stem) + ".pfm");

    unsigned done = 0;  // samples per pixel so far (the nominal count: the dumps' names)
    // --adaptive (no counterpart in the reference: the consumer of the tile-local moments): after every iteration the tiles
    // are ranked by the noise of their radiance estimate (Estimator::TileNoise: tile mean of the variance of the mean, from
    // the wave-level reduction statmc_tile_moments), and in the next iteration the noisiest quarter gets twice the
    // schedule's samples per pixel, the quietest quarter half of them (at least one).  Counts then differ from tile to tile.
    std::vector<unsigned> tileDone(nTilesTotal, 0u);      // samples per pixel so far, tile by tile
    std::vector<float> tileNoise;                          // of the last iteration (empty: no ranking yet)
    // --adaptive-pixels (no counterpart in the reference either): after every iteration but the last the NEXT iteration's
    // width * height * target samples are planned per pixel on the device from the radiance statistics as they stand
    // (Estimator::PlanSamples: statmc_sample_scores, relative metric, then statmc_plan_samples with 1 .. 4 * target samples per
    // pixel); only the count image comes back.  The tiles of the next iteration are then ragged, and Merge*Tile(s) take them as
    // they are.  Every stat type of a pixel gets the same samples.
    std::vector<int32_t> pixelTarget;                      // the plan of this iteration (empty: the schedule's target everywhere)
    std::vector<unsigned> pixelDone(o.adaptivePixels ? (size_t)width * height : 0, 0u);   // samples so far, pixel by pixel
    auto RenderLoop = [&](const int nIterations, const bool writeOutput) {
    for (int i = 1; i <= nIterations; i++) {
        const unsigned target = i == 1 ? (unsigned)o.spp : (unsigned)o.spp << std::max(i - 2, 0);  // statpath.cpp:272-279
        std::vector<unsigned> tileTarget(nTilesTotal, target);
        if (o.adaptive && !tileNoise.empty()) {
            std::vector<int> order(nTilesTotal);
            for (int t = 0; t < nTilesTotal; t++) order[t] = t;
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return tileNoise[a] < tileNoise[b]; });   // ties: tile order
            const int q = nTilesTotal / 4;
            for (int k = 0; k < q; k++) {
                tileTarget[order[k]] = std::max(1u, target / 2);
                tileTarget[order[nTilesTotal - 1 - k]] = 2 * target;
            }
        }
        auto begin = std::chrono::steady_clock::now();
        std::atomic<int> nextTile{0};
        std::atomic<bool> failed{false};
        std::string failure;
        std::mutex failMu;
        auto worker = [&]() {
            try {
                std::vector<Vec3> Ls(nLs);
                for (int t = nextTile.fetch_add(1); t < nTilesTotal; t = nextTile.fetch_add(1)) {
                    const Bounds2i tb = tileBoundsOf(t);
                    std::vector<StatTile<T>> &tileLs = lTiles[t];
                    std::vector<std::vector<StatTile<Vec3>>> &tileRGBFeatures = rgbFeatureTiles[t];
                    std::vector<std::vector<StatTile<float>>> &tileMISTallies = misTallyTiles[t];
                    if (o.closeTiles && !pixelTarget.empty()) {   // a render tile inside closed tiles: nothing to add, nothing to merge
                        bool any = false;
                        for (int y = tb.pMin.y; y < tb.pMax.y && !any; y++)
                            for (int x = tb.pMin.x; x < tb.pMax.x && !any; x++) any = pixelTarget[(size_t)y * width + x] > 0;
                        if (!any) continue;
                    }
                    for (int y = tb.pMin.y; y < tb.pMax.y; y++)
                        for (int x = tb.pMin.x; x < tb.pMax.x; x++) {
                            const Point2i actualPixel(x, y);
                            const size_t pixel = (size_t)y * width + x;
                            const unsigned target = pixelTarget.empty() ? tileTarget[t] : (unsigned)pixelTarget[pixel];   // (this pixel's)
                            const unsigned done = o.adaptivePixels ? pixelDone[pixel] : tileDone[t];
                            for (unsigned s = 0; s < target; s++) {  // do { ... } while (StartNextSample())
                                const PixelSample smp = makeSample(o.seed, x, y, done + s);
                                // Li() leaves the radiance gathered up to bounce j in Ls[j]; here a fixed share
                                for (unsigned char j = 0; j < nLs; j++) {
                                    const float share = (float)(j + 1) / (float)nLs;
                                    Ls[j] = Vec3{smp.radiance.x * share, smp.radiance.y * share, smp.radiance.z * share};
                                }
                                for (unsigned char j = sCfgs[Radiance].bounceStart; j < sCfgs[Radiance].bounceEnd; j++)
                                    (tileLs[j].*AddLSampleFn)(actualPixel, GetStatSample<T>(Ls[j]));
                                // MIS tallies per bounce: which technique won the sample (statpath.cpp:361-364)
                                for (unsigned char j = sCfgs[MISBSDFWinRate].bounceStart; j < sCfgs[MISBSDFWinRate].bounceEnd; j++) {
                                    const float bsdf = (float)((draw(o.seed, x, y, done + s, 20u + j) >> 3) & 1u);
                                    const float light = (float)((draw(o.seed, x, y, done + s, 40u + j) >> 3) & 1u);
                                    (tileMISTallies[j][0].*AddMISWinRateSampleFn)(actualPixel, bsdf);
                                    (tileMISTallies[j][1].*AddMISWinRateSampleFn)(actualPixel, light);
                                }
                                (tileRGBFeatures[0][0].*AddRGBGBufferSampleFn)(actualPixel, smp.normal);
                                (tileRGBFeatures[0][1].*AddRGBGBufferSampleFn)(actualPixel, smp.albedo);
                            }
                        }
                    // Merge tiles into buffers (statpath.cpp:381-388)
                    if (sCfgs[Radiance].enable) estimator.MergeTransformTiles(tileLs, sCfgs[Radiance]);
                    if (misEnabled) estimator.MergeTiles(tileMISTallies, misCfgs);
                    estimator.MergeTiles(tileRGBFeatures, enabledRGBFeatureCfgs);
                }
            } catch (const std::exception &e) {
                std::lock_guard<std::mutex> lk(failMu);
                failed = true;
                failure = e.what();
            }
        };
        std::vector<std::thread> pool;
        for (int t = 0; t < o.threads; t++) pool.emplace_back(worker);
        for (auto &t : pool) t.join();
        if (failed) throw std::runtime_error(failure);
        done += target;
        for (int t = 0; t < nTilesTotal; t++) tileDone[t] += tileTarget[t];
        if (o.adaptivePixels) {
            unsigned long long spent = 0;
            for (size_t p = 0; p < pixelDone.size(); p++) {
                const unsigned c = pixelTarget.empty() ? target : (unsigned)pixelTarget[p];
                pixelDone[p] += c;
                spent += c;
            }
            std::cout << "Target: " << target << " spp" << std::endl;
            std::cout << "Spent: " << spent << " samples" << std::endl;
        }
        auto end = std::chrono::steady_clock::now();
        std::cout << "Iteration: " << i << std::endl;
        std::cout << "SPP: " << target << std::endl;
        std::cout << "Rendering time [ns]: " << std::chrono::duration_cast<std::chrono::nanoseconds>(end - begin).count() << std::endl;

        begin = std::chrono::steady_clock::now();
        estimator.Upload();  // stages + accumulates the iteration's samples on the device
        if (estimator.runCUDA) {
            if (o.preview && i < nIterations) estimator.DenoisePreview(*coarseEst, o.preview);
            else estimator.Denoise();
            estimator.Download();
        }
        estimator.Synchronize();
        end = std::chrono::steady_clock::now();
        std::cout << "CUDA time [ns]: " << std::chrono::duration_cast<std::chrono::nanoseconds>(end - begin).count() << std::endl;
        if (o.adaptive && sCfgs[Radiance].enable) {
            tileNoise = estimator.TileNoise(sCfgs[Radiance].index, 0, tileSize);
            unsigned lo = ~0u, hi = 0;
            for (unsigned v : tileDone) { lo = std::min(lo, v); hi = std::max(hi, v); }
            std::cout << "Adaptive: samples per pixel so far " << lo << " .. " << hi << " over " << nTilesTotal << " tiles" << std::endl;
        }

        const char *what = o.stopMetric == Estimator::ScoreOfStdErr ? "standard error" : o.stopMetric == Estimator::ScoreOfCI ? "confidence half-width" : "score";
        // --stop-mean: the mean or RMS of the relative score under the cap, one 152-byte struct back; the divisions are done here
        bool meanMet = true;
        if (o.stopMean && sCfgs[Radiance].enable) {
            statmc_sum_result sum;
            check(statmc_download(&sum, estimator.ScoreSum(sCfgs[Radiance].index, 0, {o.stopMeanCap}, STATMC_SCORE_RELATIVE, 1e-3f, o.scoreDilate, o.stopMetric), sizeof(sum), estimator.DeviceStream()));
            estimator.Synchronize();
            const int64_t judged = sum.n_px - (sum.cap_bits[0] == 0x7F800000u ? sum.n_infinite : 0);
            const double v = judged ? (o.stopMeanRms ? std::sqrt(sum.sum_sq[0] / (double)judged) : sum.sum[0] / (double)judged) : (double)NAN;
            meanMet = v <= (double)o.stopMeanTarget;   // (no judged pixel: not met)
            char value[32], cap[32], target[32];
            std::snprintf(value, sizeof(value), "%.9g", v);
            std::snprintf(cap, sizeof(cap), "%.9g", (double)o.stopMeanCap);
            std::snprintf(target, sizeof(target), "%.9g", (double)o.stopMeanTarget);
            std::cout << "Mean rule: iteration " << i << ", " << (o.stopMeanRms ? "rms" : "mean") << " of the relative " << what << " under " << cap << " = "
                      << value << " over " << judged << " pixels, target " << target << ": " << (meanMet ? "met" : "open") << std::endl;
        }

        // --stop-tiles: the tiles whose mean relative score under the cap is above the tolerance, one int64 back
        bool tilesMet = true;
        const float *tileRulePlane = nullptr;   // --close-tiles: what the gate of this iteration and of the next plan reads
        if (o.stopTiles && o.tileQuantile && sCfgs[Radiance].enable) {
            const statmc_tile_quantiles planes = estimator.ScoreTileQuantiles(sCfgs[Radiance].index, 0, o.stopTilesTile, {o.tileQuantileNum}, o.tileQuantileDen,
                                                                             o.scoreDilate, o.stopMetric);
            tileRulePlane = planes.value[0];
            const int tilesX = Estimator::TilesAcross(width, o.stopTilesTile), tilesY = Estimator::TilesAcross(height, o.stopTilesTile);
            const float tol = o.stopTilesTol;
            int64_t *d_open = estimator.TileRuleCount();
            check(statmc_score_count_above((uint16_t)tilesX, (uint16_t)tilesY, planes.value[0], &tol, 1, d_open, estimator.DeviceStream()));
            int64_t open = 0;
            check(statmc_download(&open, d_open, sizeof(open), estimator.DeviceStream()));
            estimator.Synchronize();
            tilesMet = open == 0;
            char tolerance[32];
            std::snprintf(tolerance, sizeof(tolerance), "%.9g", (double)o.stopTilesTol);
            std::cout << "Tile rule: iteration " << i << ", open tiles " << open << " / " << (int64_t)tilesX * tilesY << " of " << o.stopTilesTile << " x "
                      << o.stopTilesTile << " pixels, quantile " << o.tileQuantileNum << "/" << o.tileQuantileDen << " of the relative " << what << " above "
                      << tolerance << ": " << (tilesMet ? "met" : "open") << std::endl;
        } else if (o.stopTiles && sCfgs[Radiance].enable) {
            const statmc_tile_scores planes = estimator.ScoreTiles(sCfgs[Radiance].index, 0, o.stopTilesTile, o.stopTilesCap, o.scoreDilate, o.stopMetric);
            tileRulePlane = planes.mean;
            const int tilesX = Estimator::TilesAcross(width, o.stopTilesTile), tilesY = Estimator::TilesAcross(height, o.stopTilesTile);
            const float tol = o.stopTilesTol;
            int64_t *d_open = estimator.TileRuleCount();
            check(statmc_score_count_above((uint16_t)tilesX, (uint16_t)tilesY, planes.mean, &tol, 1, d_open, estimator.DeviceStream()));
            int64_t open = 0;
            check(statmc_download(&open, d_open, sizeof(open), estimator.DeviceStream()));
            estimator.Synchronize();
            tilesMet = open == 0;
            char cap[32], tolerance[32];
            std::snprintf(cap, sizeof(cap), "%.9g", (double)o.stopTilesCap);
            std::snprintf(tolerance, sizeof(tolerance), "%.9g", (double)o.stopTilesTol);
            std::cout << "Tile rule: iteration " << i << ", open tiles " << open << " / " << (int64_t)tilesX * tilesY << " of " << o.stopTilesTile << " x "
                      << o.stopTilesTile << " pixels, mean of the relative " << what << " under " << cap << " above " << tolerance << ": "
                      << (tilesMet ? "met" : "open") << std::endl;
        }
        // --close-tiles: the rule's plane through the gate, with the closed plane of the run; a tile closed earlier stays closed
        Estimator::TileGate tileGate{o.stopTilesTile, tileRulePlane, o.stopTilesTol, nullptr, nullptr};
        if (o.closeTiles && tileRulePlane) {
            const Estimator::TileGatePlanes gp = estimator.GatePlanes(o.stopTilesTile);
            tileGate.d_closed = gp.d_closed, tileGate.d_open = gp.d_open;
            const statmc_gate_result g = estimator.GateTiles(o.stopTilesTile, tileRulePlane, o.stopTilesTol, gp.d_closed, gp.d_open);
            tilesMet = g.n_open == 0;
            std::cout << "Closed tiles: iteration " << i << ", closed now " << g.n_closed_now << ", open " << g.n_open << " / " << g.n_tiles
                      << ", open pixels " << g.n_px_open << std::endl;
        }

        // --stop-at: the Q-quantile of the relative score, one 256-byte struct back
        bool converged = (o.stopMean || o.stopTiles) && !o.stopAt && meanMet && tilesMet && sCfgs[Radiance].enable;
        if (o.stopAt && sCfgs[Radiance].enable) {
            const int64_t rank = Estimator::NearestRank(o.stopQuantile, (int64_t)width * height);
            statmc_select_result sel;
            check(statmc_download(&sel, estimator.ScoreSelect(sCfgs[Radiance].index, 0, {rank}, STATMC_SCORE_RELATIVE, 1e-3f, o.scoreDilate, o.stopMetric), sizeof(sel), estimator.DeviceStream()));
            estimator.Synchronize();
            float v;
            std::memcpy(&v, &sel.value_bits[0], sizeof(v));
            char value[32];
            std::snprintf(value, sizeof(value), "%.9g", (double)v);
            if (o.stopMetric != Estimator::ScoreOfDeviation)
                std::cout << "Stop metric: iteration " << i << ", quantile " << o.stopQuantile << " of the relative " << what << " = " << value << std::endl;
            if (v <= o.stopThreshold && meanMet && tilesMet) {
                converged = true;
                std::cout << "Converged: iteration " << i << ", quantile " << o.stopQuantile << " of the relative " << what << " = " << value << std::endl;
            }
        }

        if (o.adaptivePixels && o.targetErrorGiven && sCfgs[Radiance].enable && i < nIterations && !converged) {
            const unsigned next = (unsigned)o.spp << std::max(i - 1, 0);   // the schedule's target of iteration i + 1
            const int scoreOf = o.stopMetric == Estimator::ScoreOfDeviation ? (int)Estimator::ScoreOfCI : o.stopMetric;
            const Estimator::TargetPlan plan = estimator.PlanToTarget(sCfgs[Radiance].index, 0, o.targetError, (int64_t)width * height * next, 1,
                                                                      (int32_t)(4 * next), STATMC_SCORE_RELATIVE, 1e-3f, scoreOf, o.scoreDilate);
            pixelTarget.resize((size_t)width * height);
            check(statmc_download(pixelTarget.data(), plan.d_counts, pixelTarget.size() * sizeof(int32_t), estimator.DeviceStream()));
            estimator.Synchronize();
            std::cout << "Planned to target: total " << plan.target.total << ", need " << plan.target.need << ", n_open " << plan.target.n_open
                      << ", n_capped " << plan.target.n_capped << ", by " << (plan.byBudget ? "budget" : "target") << std::endl;
            if (plan.byBudget) {
                int32_t lo = pixelTarget[0], hi = pixelTarget[0];
                for (int32_t v : pixelTarget) { lo = std::min(lo, v); hi = std::max(hi, v); }
                char level[16];
                std::snprintf(level, sizeof(level), "%08x", (unsigned)plan.budgeted.level_bits);
                std::cout << "Planned: " << plan.budgeted.total << " samples, " << lo << " .. " << hi << " per pixel, level 0x" << level << std::endl;
            }
        } else if (o.adaptivePixels && o.closeTiles && tileRulePlane && i < nIterations && !converged) {
            const unsigned next = (unsigned)o.spp << std::max(i - 1, 0);   // the schedule's target of iteration i + 1
            const Estimator::GatedPlan plan = estimator.PlanSamples(sCfgs[Radiance].index, 0, tileGate, (int64_t)next, 0, (int32_t)(4 * next),
                                                                    STATMC_SCORE_RELATIVE, 1e-3f, o.scoreDilate);
            pixelTarget.resize((size_t)width * height);
            check(statmc_download(pixelTarget.data(), plan.d_counts, pixelTarget.size() * sizeof(int32_t), estimator.DeviceStream()));
            estimator.Synchronize();
            int32_t lo = pixelTarget[0], hi = pixelTarget[0];
            for (int32_t v : pixelTarget) { lo = std::min(lo, v); hi = std::max(hi, v); }
            char level[16];
            std::snprintf(level, sizeof(level), "%08x", (unsigned)plan.result.level_bits);
            std::cout << "Planned: " << plan.result.total << " samples, " << lo << " .. " << hi << " per pixel, level 0x" << level << std::endl;
        } else if (o.adaptivePixels && sCfgs[Radiance].enable && i < nIterations && !converged) {
            const unsigned next = (unsigned)o.spp << std::max(i - 1, 0);   // the schedule's target of iteration i + 1
            const Estimator::SamplePlan plan = estimator.PlanSamples(sCfgs[Radiance].index, 0, (int64_t)width * height * next, 1, (int32_t)(4 * next),
                                                                     STATMC_SCORE_RELATIVE, 1e-3f, o.scoreDilate);
            pixelTarget.resize((size_t)width * height);
            check(statmc_download(pixelTarget.data(), plan.d_counts, pixelTarget.size() * sizeof(int32_t), estimator.DeviceStream()));
            estimator.Synchronize();
            int32_t lo = pixelTarget[0], hi = pixelTarget[0];
            for (int32_t v : pixelTarget) { lo = std::min(lo, v); hi = std::max(hi, v); }
            char level[16];
            std::snprintf(level, sizeof(level), "%08x", (unsigned)plan.result.level_bits);
            std::cout << "Planned: " << plan.result.total << " samples, " << lo << " .. " << hi << " per pixel, level 0x" << level << std::endl;
        }

        begin = std::chrono::steady_clock::now();
        if (!o.stem.empty() && writeOutput) {  // statpath.cpp:419-427: outBufSel.PrepareOutput(); outBufSel.Write(total spp)
            // what lives only on the device comes to the host mats first: the statistics, and the
            // filter's device-only by-products (mean-corr, discriminator)
            estimator.DownloadStatistics();
            if (estimator.runCUDA)
                for (auto *bufs : {&estimator.meanCorrBuffers, &estimator.discriminatorBuffers})
                    for (auto &perType : *bufs)
                        for (Buffer &b : perType) b.download(estimator.stream);
            estimator.Synchronize();
            outBufSel.PrepareOutput();
            outBufSel.Write(std::to_string(done));
            if (o.tileStats && !estimator.filmBuffers.empty() && !estimator.filmBuffers[0].empty()) {
                // --tilestats: the local noise level of the radiance estimate, one value per 16 x 16 tile (the tile
                // size of the render loop): "<stem>-<spp>-t0-b0-tile-mean.pfm" and "-tile-var.pfm" (pooled sample
                // variance M2 / (count - 1) of the per-pixel means inside the tile), from wave-level reductions
                const Buffer &fm = estimator.filmBuffers[0][0];
                const int C = fm.gpuMat.channels();
                const HostImage tm = estimator.TileMoments(fm, 16);
                const int ty = tm.rows, tx = tm.cols / C;
                std::vector<float> mean((size_t)ty * tx * C), var((size_t)ty * tx * C);
                float worst = -1.f;
                int wx = 0, wy = 0;
                for (int y = 0; y < ty; y++)
                    for (int x = 0; x < tx; x++)
                        for (int c = 0; c < C; c++) {
                            const float *m = tm.ptr<float>() + (((size_t)y * tx + x) * C + c) * 3;
                            const size_t k = ((size_t)y * tx + x) * C + c;
                            mean[k] = m[1];
                            var[k] = m[0] > 1.f ? m[2] / (m[0] - 1.f) : 0.f;
                            if (var[k] > worst) { worst = var[k]; wx = x; wy = y; }
                        }
                const std::string prefix = o.stem + "-" + std::to_string(done) + "-" + fm.name + "-";
                writePfm(prefix.substr(0, prefix.size() - std::string("film-mean-").size()) + "tile-mean.pfm", tx, ty, C, mean.data());
                writePfm(prefix.substr(0, prefix.size() - std::string("film-mean-").size()) + "tile-var.pfm", tx, ty, C, var.data());
                std::cout << "Noisiest tile: (" << wx << ", " << wy << ") variance " << worst << std::endl;
            }
        }
        end = std::chrono::steady_clock::now();
        std::cout << "Output time [ns]: " << std::chrono::duration_cast<std::chrono::nanoseconds>(end - begin).count() << std::endl;
        if (converged) break;
    }
    };

    if (o.warmUp) {  // statpath.cpp:433-437: one throw-away iteration, then everything starts over
        std::cout << "==== Warm-Up Start ====" << std::endl;
        RenderLoop(1, false);
        std::cout << "==== Warm-Up End ====" << std::endl;
        // the reference re-creates its tiles, i.e. all statistics, for the real run
        for (unsigned char t = 0; t < estimator.statTypeConfigs.nEnabled; t++) estimator.ResetStatistics(t);
        done = 0;
        std::fill(tileDone.begin(), tileDone.end(), 0u);
        tileNoise.clear();
        pixelTarget.clear();
        std::fill(pixelDone.begin(), pixelDone.end(), 0u);
    }
    RenderLoop(o.iterations, true);
    std::cout << "Staged bytes: " << estimator.stagedBytes() << std::endl;   // sample bytes handed to the device, warm-up included
}

int main(int argc, char **argv) {
    Options o;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> const char * {
            if (i + 1 >= argc) {
                std::fprintf(stderr, "missing value for %s\n", a.c_str());
                std::exit(2);
            }
            return argv[++i];
        };
        if (a == "--width") o.width = std::atoi(next());
        else if (a == "--height") o.height = std::atoi(next());
        else if (a == "--spp") o.spp = std::atoi(next());
        else if (a == "--iterations") o.iterations = std::atoi(next());
        else if (a == "--threads") o.threads = std::atoi(next());
        else if (a == "--seed") o.seed = (unsigned)std::strtoul(next(), nullptr, 10);
        else if (a == "--filtersd") o.filterSD = (float)std::atof(next());
        else if (a == "--filterradius") o.filterRadius = std::atoi(next());
        else if (a == "--stage-mb") o.stageMb = std::atoi(next());
        else if (a == "--trackedbounces") o.trackedBounces = std::atoi(next());
        else if (a == "--stem") o.stem = next();
        else if (a == "--outputregex") o.outputRegex = next();
        else if (a == "--no-denoise") o.denoise = false;
        else if (a == "--warmup") o.warmUp = true;
        else if (a == "--tilestats") o.tileStats = true;
        else if (a == "--adaptive") o.adaptive = true;
        else if (a == "--adaptive-pixels") o.adaptivePixels = true;
        else if (a == "--stop-at") {
            const std::string v = next();
            const size_t colon = v.find(':');
            char *end = nullptr;
            if (colon != std::string::npos) {
                o.stopQuantile = std::strtod(v.c_str(), &end);
                o.stopAt = end == v.c_str() + colon && colon > 0;
                o.stopThreshold = std::strtof(v.c_str() + colon + 1, &end);
                o.stopAt = o.stopAt && *end == 0 && end != v.c_str() + colon + 1;
            }
            if (!o.stopAt || !(o.stopQuantile >= 0.0 && o.stopQuantile <= 1.0) || o.stopThreshold != o.stopThreshold) {
                std::fprintf(stderr, "--stop-at takes Q:T, a quantile in [0, 1] and a threshold\n");
                return 2;
            }
        } else if (a == "--stop-mean") {
            const std::string v = next();
            const size_t c1 = v.find(':'), c2 = c1 == std::string::npos ? c1 : v.find(':', c1 + 1);
            const std::string rule = v.substr(0, c1);
            char *end = nullptr;
            bool ok = c1 != std::string::npos && (rule == "mean" || rule == "rms");
            if (ok) {
                const std::string t = v.substr(c1 + 1, c2 == std::string::npos ? c2 : c2 - c1 - 1);
                o.stopMeanTarget = std::strtof(t.c_str(), &end);
                ok = !t.empty() && *end == 0 && o.stopMeanTarget >= 0.f;   // (a NaN fails the comparison)
            }
            if (ok && c2 != std::string::npos) {
                const std::string c = v.substr(c2 + 1);
                o.stopMeanCap = std::strtof(c.c_str(), &end);
                ok = !c.empty() && *end == 0 && o.stopMeanCap == o.stopMeanCap;
            }
            if (!ok) {
                std::fprintf(stderr, "--stop-mean takes mean:T, rms:T or either with :CAP, a target >= 0 and a cap that is not NaN\n");
                return 2;
            }
            o.stopMean = true;
            o.stopMeanRms = rule == "rms";
        } else if (a == "--stop-tiles") {
            const std::string v = next();
            const size_t c1 = v.find(':'), c2 = c1 == std::string::npos ? c1 : v.find(':', c1 + 1);
            char *end = nullptr;
            bool ok = c1 != std::string::npos;
            if (ok) {
                const std::string t = v.substr(0, c1);
                const long tile = std::strtol(t.c_str(), &end, 10);
                ok = !t.empty() && *end == 0 && (tile == 8 || tile == 16 || tile == 32 || tile == 64);
                o.stopTilesTile = (int)tile;
            }
            if (ok) {
                const std::string t = v.substr(c1 + 1, c2 == std::string::npos ? c2 : c2 - c1 - 1);
                o.stopTilesTol = std::strtof(t.c_str(), &end);
                ok = !t.empty() && *end == 0 && o.stopTilesTol >= 0.f;   // (a NaN fails the comparison)
            }
            if (ok && c2 != std::string::npos) {
                const std::string c = v.substr(c2 + 1);
                o.stopTilesCap = std::strtof(c.c_str(), &end);
                ok = !c.empty() && *end == 0 && o.stopTilesCap == o.stopTilesCap;
            }
            if (!ok) {
                std::fprintf(stderr, "--stop-tiles takes T:TOL or T:TOL:CAP, a tile of 8, 16, 32 or 64, a tolerance >= 0 and a cap that is not NaN\n");
                return 2;
            }
            o.stopTiles = true;
        } else if (a == "--tile-quantile") {
            const std::string v = next();
            const size_t slash = v.find('/');
            char *end = nullptr;
            bool ok = slash != std::string::npos && slash > 0 && slash + 1 < v.size();
            if (ok) {
                const std::string n = v.substr(0, slash), d = v.substr(slash + 1);
                const long num = std::strtol(n.c_str(), &end, 10);
                ok = *end == 0;
                const long den = std::strtol(d.c_str(), &end, 10);
                ok = ok && *end == 0 && den >= 1 && den <= 65536 && num >= 0 && num <= den;
                o.tileQuantileNum = (int)num, o.tileQuantileDen = (int)den;
            }
            if (!ok) {
                std::fprintf(stderr, "--tile-quantile takes NUM/DEN with 0 <= NUM <= DEN and 1 <= DEN <= 65536\n");
                return 2;
            }
            o.tileQuantile = true;
        } else if (a == "--close-tiles") {
            o.closeTiles = true;
        } else if (a == "--stop-metric") {
            const std::string v = next();
            if (v != "sd" && v != "stderr" && v != "ci") {
                std::fprintf(stderr, "--stop-metric takes sd, stderr or ci\n");
                return 2;
            }
            o.stopMetricGiven = true;
            o.stopMetric = v == "sd" ? Estimator::ScoreOfDeviation : v == "stderr" ? Estimator::ScoreOfStdErr : Estimator::ScoreOfCI;
        } else if (a == "--preview") {
            o.preview = std::atoi(next());
            if (o.preview != 2 && o.preview != 4 && o.preview != 8) {
                std::fprintf(stderr, "--preview 2 | 4 | 8\n");
                return 2;
            }
        } else if (a == "--target-error") {
            const std::string v = next();
            char *end = nullptr;
            o.targetError = std::strtof(v.c_str(), &end);
            if (v.empty() || *end != 0 || !(o.targetError >= 0x1p-60f && o.targetError <= 0x1p60f)) {
                std::fprintf(stderr, "--target-error takes a tolerance in [2^-60, 2^60]\n");
                return 2;
            }
            o.targetErrorGiven = true;
        } else if (a == "--score-dilate") {
            const std::string v = next();
            char *end = nullptr;
            const long r = std::strtol(v.c_str(), &end, 10);
            if (v.empty() || *end != 0 || r < 0 || r > STATMC_SCORE_WINDOW_MAX_RADIUS) {
                std::fprintf(stderr, "--score-dilate takes a radius, 0 to %d\n", STATMC_SCORE_WINDOW_MAX_RADIUS);
                return 2;
            }
            o.scoreDilateGiven = true;
            o.scoreDilate = (int)r;
        } else if (a == "--half-features") o.halfFeatures = true;
        else if (a == "--placed") statmc::usePlacedMemory() = true;   // device images and sample arenas from statmc_malloc_placed
        else if (a == "--config") {
            const std::string c = next();
            if (c != "denoise" && c != "acrr" && c != "smis") {
                std::fprintf(stderr, "unknown config %s\n", c.c_str());
                return 2;
            }
            o.acrr = c == "acrr";
            o.smis = c == "smis";
        } else if (a == "--print-sample") {  // x y s: the generator alone, no device (CPU test of the restatement)
            const int x = std::atoi(next()), y = std::atoi(next());
            const unsigned s = (unsigned)std::strtoul(next(), nullptr, 10);
            const PixelSample p = makeSample(o.seed, x, y, s);
            std::printf("%a %a %a %a %a %a %a %a %a\n", p.radiance.x, p.radiance.y, p.radiance.z, p.normal.x, p.normal.y,
                        p.normal.z, p.albedo.x, p.albedo.y, p.albedo.z);
            return 0;
        } else {
            std::fprintf(stderr, "unknown option %s\n", a.c_str());
            return 2;
        }
    }
    if (o.width <= 0 || o.height <= 0 || o.width > 65535 || o.height > 65535 || o.spp <= 0 || o.iterations <= 0 ||
        o.threads <= 0 || o.trackedBounces < 1 || o.trackedBounces > 16) {
        std::fprintf(stderr, "bad size / spp / iterations / threads / trackedbounces\n");
        return 2;
    }
    if (o.preview && o.stopAt) {
        std::fprintf(stderr, "--preview cannot be used with --stop-at (the last iteration is denoised in full, and --stop-at decides it late)\n");
        return 2;
    }
    if (o.preview && o.stopMean) {
        std::fprintf(stderr, "--preview cannot be used with --stop-mean (the last iteration is denoised in full, and --stop-mean decides it late)\n");
        return 2;
    }
    if (o.preview && o.stopTiles) {
        std::fprintf(stderr, "--preview cannot be used with --stop-tiles (the last iteration is denoised in full, and --stop-tiles decides it late)\n");
        return 2;
    }
    if ((o.tileQuantile || o.closeTiles) && !o.stopTiles) {
        std::fprintf(stderr, "--tile-quantile and --close-tiles need --stop-tiles\n");
        return 2;
    }
    if (o.closeTiles && o.targetErrorGiven) {
        std::fprintf(stderr, "--close-tiles cannot be used with --target-error (the gated plan spends a budget)\n");
        return 2;
    }
    if (o.stopTiles && !o.adaptivePixels) {
        std::fprintf(stderr, "--stop-tiles needs --adaptive-pixels\n");
        return 2;
    }
    if (o.stopMean && !o.adaptivePixels) {
        std::fprintf(stderr, "--stop-mean needs --adaptive-pixels\n");
        return 2;
    }
    if (o.stopAt && !o.adaptivePixels) {
        std::fprintf(stderr, "--stop-at needs --adaptive-pixels\n");
        return 2;
    }
    if ((o.stopMetricGiven || o.targetErrorGiven) && !o.adaptivePixels) {
        std::fprintf(stderr, "--stop-metric and --target-error need --adaptive-pixels\n");
        return 2;
    }
    if (o.scoreDilateGiven && !o.adaptivePixels) {
        std::fprintf(stderr, "--score-dilate needs --adaptive-pixels\n");
        return 2;
    }
    try {
        if (o.acrr) Render<float>(o);  // StatPathIntegrator::Render dispatches on enableMultiChannelStats
        else Render<Vec3>(o);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "statmc_render_sim: %s\n", e.what());
        return 1;
    }
    return 0;
}
