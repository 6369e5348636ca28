// Host section of ssamd_api.hip: the per-shape geometry caches around the planners and the autotuner's bookkeeping (ASW and GSW).
namespace {
// Locking: every device has its own context and its own mutex (Ctx::mu), so one process can drive several GPUs
// concurrently through the operators (ssamd_*_multi does, one host thread per device).  g_geom_mutex guards the
// small process-wide launch-geometry caches only and is never held across a HIP call.
std::mutex g_geom_mutex;

// The planners are functions of their arguments and know no error codes: their verdicts become the operators' errors here.
int asw_search(AswGeom &best, const PlanOptions &po, int W, int rows, int win, int nD, std::vector<AswGeom> *shortlist = nullptr)
{
    const PlanResult r = asw_search_geometry(best, po, W, rows, win, nD, shortlist);
    if (r == PLAN_FORCED_UNUSABLE) return fail(SSAMD_ELIMIT, "SSAMD_ASW_GEOM does not fit LDS");
    return r == PLAN_OK ? SSAMD_OK : fail(SSAMD_ELIMIT, "no ASW launch geometry fits LDS for winSize=%d nD=%d", win, nD);
}

int gsw_search(GswGeom &best, const std::string &forced, int W, int rows, int win, int nD)
{
    const PlanResult r = gsw_search_geometry(best, forced, W, rows, win, nD);
    if (r == PLAN_FORCED_UNUSABLE) return fail(SSAMD_EINVAL, "SSAMD_GSW_GEOM=%s is not a usable geometry", forced.c_str());
    return r == PLAN_OK ? SSAMD_OK : fail(SSAMD_ELIMIT, "no GSW launch geometry fits LDS for winSize=%d nD=%d", win, nD);
}

// The search walks a few thousand candidate tiles (0.1-0.3 ms on the host): remember the answer per problem shape,
// a video stream asks the same question every frame.  (All four maps are guarded by g_geom_mutex.)
using ShapeKey = std::array<int, 4>;      // W, workgroup rows, winSize, nD
template <class Geom> struct GeomCache {
    std::map<ShapeKey, Geom> geom;
    std::map<ShapeKey, bool> tuned;       // shapes whose cached geometry was picked by measurement
};
GeomCache<AswGeom> g_asw_geom;
GeomCache<GswGeom> g_gsw_geom;
// autotuning mode: 1 always, 0 never, -1 (default) only for small problems, where the ~50 trial launches cost
// at most about 0.4 s once and where the cost model is least reliable
std::atomic<int> g_autotune{g_tuning.autotune_env != -2 ? g_tuning.autotune_env : -1};
constexpr double ASW_AUTOTUNE_SMALL_TAPS = 6.0e10;      // window taps per call (about 6-8 ms of kernel time; 3e10 until round 4)

// forced (tuning hooks: asw_geometry_forced, SSAMD_GSW_GEOM): never cached
template <class Geom, class Search>
int choose_geometry(GeomCache<Geom> &cache, bool forced, const ShapeKey &key, Geom &best, Search search)
{
    if (forced) return search(best);
    std::lock_guard<std::mutex> glk(g_geom_mutex);
    auto it = cache.geom.find(key);
    if (it != cache.geom.end()) { best = it->second; return SSAMD_OK; }
    const int rc = search(best);
    if (rc == SSAMD_OK) {
        if (cache.geom.size() > 256) { cache.geom.clear(); cache.tuned.clear(); }
        cache.geom[key] = best;
    }
    return rc;
}

int asw_choose_geometry(AswGeom &best, const PlanOptions &po, int W, int rows, int win, int nD)
{
    return choose_geometry(g_asw_geom, asw_geometry_forced(po.t), {W, rows, win, nD}, best,
                           [&](AswGeom &g) { return asw_search(g, po, W, rows, win, nD); });
}

int gsw_choose_geometry(GswGeom &best, const Tuning &t, int W, int rows, int win, int nD)
{
    return choose_geometry(g_gsw_geom, !t.gsw_geom.empty(), {W, rows, win, nD}, best,
                           [&](GswGeom &g) { return gsw_search(g, t.gsw_geom, W, rows, win, nD); });
}

// Autotuning (ssamd_autotune): is this call the one that times the candidates of its shape?
template <class Geom> bool autotune_due(GeomCache<Geom> &cache, const ShapeKey &shape, double call_taps)
{
    const int mode = g_autotune.load();
    std::lock_guard<std::mutex> glk(g_geom_mutex);
    return (mode > 0 || (mode < 0 && call_taps <= ASW_AUTOTUNE_SMALL_TAPS)) && cache.tuned.count(shape) == 0;
}
// ... the trial launches: round-robin over the n candidates, `rounds` rounds, fastest launch of each (round 0 is warm-up) -- clocks
// ramp up during the first launches after an idle period, so timing the candidates one after the other would favour the late ones.
// run(ci) prepares and launches candidate ci; anything that fails costs it the round (and clears *ok, when asked).
// prune: a candidate that is twice as slow as the best one in the warm-up round (very narrow tiles can be several times slower than
// the model's choice) is not timed again: bounds what the first call of a shape costs.
// The verdict: the model's own choice (first) keeps the job unless another candidate is clearly faster.  -1: none was timed
template <class Run> int autotune_rounds(size_t n, int rounds, bool prune, hipEvent_t e0, hipEvent_t e1, hipStream_t s, bool *ok, Run run)
{
    std::vector<float> cand_ms(n, 3.0e38f), warm_ms(n, 3.0e38f);
    std::vector<char> alive(n, 1);
    for (int round = 0; round < rounds; ++round) {
        for (size_t ci = 0; ci < n; ++ci) {
            if (!alive[ci]) continue;
            float ms = 3.0e38f;
            if (hipEventRecord(e0, s) == hipSuccess && run(ci) && hipEventRecord(e1, s) == hipSuccess && hipEventSynchronize(e1) == hipSuccess)
                (void)hipEventElapsedTime(&ms, e0, e1);
            else if (ok)
                *ok = false;
            if (round > 0) cand_ms[ci] = std::min(cand_ms[ci], ms);
            else warm_ms[ci] = ms;
        }
        if (round == 0 && prune) {
            const float wbest = *std::min_element(warm_ms.begin(), warm_ms.end());
            for (size_t ci = 1; ci < n; ++ci) alive[ci] = warm_ms[ci] <= 2.0f * wbest;
        }
    }
    int fastest = -1;
    float best_ms = 3.0e38f;
    for (size_t ci = 0; ci < n; ++ci)
        if (cand_ms[ci] < best_ms * (ci == 0 ? 1.0f : 0.985f)) { best_ms = cand_ms[ci]; fastest = (int)ci; }
    return fastest;
}
template <class Geom> void autotune_keep(GeomCache<Geom> &cache, const ShapeKey &shape, const Geom &fastest)
{
    std::lock_guard<std::mutex> glk(g_geom_mutex);
    cache.geom[shape] = fastest;
    cache.tuned[shape] = true;
}
}  // namespace
