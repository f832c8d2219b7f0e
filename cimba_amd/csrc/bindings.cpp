// pybind11 bindings for cimba_amd.
//
// The Python layer is orchestration only (bench harness, distributed
// experiment fan-out via torch.distributed/RCCL); the engine, executive and
// kernels are native C++/HIP (SURVEY.md §2.1 native-code census).
#include <pybind11/pybind11.h>
#include <pybind11/numpy.h>
#include <pybind11/stl.h>

#include "cimba/bulk_rng.hpp"
#include "cimba/dataset.hpp"
#include "cimba/heapfuzz.hpp"
#include "cimba/logger.hpp"
#include "cimba/runner.hpp"
#include "cimba/stats.hpp"
#include "cimba/terrain.hpp"
#include "../models/mm1.hpp"
#include "../models/mm1_logged.hpp"
#include "../models/mm1_tally.hpp"
#include "../models/mg1.hpp"
#include "../models/jobshop.hpp"
#include "../models/awacs.hpp"
#include "../models/scenarios.hpp"
#include "../models/spillprobe.hpp"

#include <atomic>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace py = pybind11;
using namespace cmb;
using cmb_models::MM1;

// from hip/deskernel.hip
extern "C" {
struct Mm1GpuOut {
    double elapsed_ms;
    uint64_t total_events;
    uint64_t total_objs;
    double total_wait;
    uint64_t trials_ok;
    int32_t first_bad_status;
    int32_t pad_;
};
int cimba_mm1_gpu_run(uint64_t ntrials, double arr_mean, double srv_mean,
                      uint64_t num_objects, uint64_t seed,
                      uint64_t trial_base, int device, double until,
                      uint64_t max_events, Mm1GpuOut* out);
int cimba_mm1_gpu_run_pt(uint64_t ntrials, double arr_mean, double srv_mean,
                         uint64_t num_objects, uint64_t seed,
                         uint64_t trial_base, int device, double until,
                         uint64_t max_events, Mm1GpuOut* out,
                         double* per_trial_avg_out);
// from hip/deskernel_mm1hot1.hip
int cimba_mm1hot1_gpu_run_pt(uint64_t ntrials, double arr_mean,
                             double srv_mean, uint64_t num_objects,
                             uint64_t seed, uint64_t trial_base, int device,
                             double until, uint64_t max_events, Mm1GpuOut* out,
                             double* per_trial_avg_out);
// from hip/deskernel_mm1rec.hip
int cimba_mm1rec_gpu_run_pt(uint64_t ntrials, double arr_mean,
                            double srv_mean, uint64_t num_objects,
                            uint64_t seed, uint64_t trial_base, int device,
                            int lane_mode, Mm1GpuOut* out,
                            double* per_trial_avg_out);
// from hip/deskernel.hip and hip/deskernel_mg1.hip
void cimba_mm1_lds_layout(uint32_t out3[3]);
void cimba_mg1_lds_layout(uint32_t out3[3]);
// from hip/deskernel_mm1log.hip
int cimba_mm1log_gpu_run(uint64_t ntrials, double arr_mean, double srv_mean,
                         uint64_t num_objects, uint64_t seed,
                         uint64_t trial_base, int device, int kernel,
                         uint32_t blocks, const cmb::LogSink* log_sink,
                         double* elapsed_ms, void* results_out);
// from hip/deskernel_mm1tally.hip
int cimba_mm1tally_gpu_run(uint64_t ntrials, double arr_mean, double srv_mean,
                           uint64_t num_objects, uint64_t seed,
                           uint64_t trial_base, int device, int kernel,
                           uint32_t blocks, cmb::TallyRequest* tally_sink,
                           double* elapsed_ms, void* results_out);
// from hip/tally_kernel.hip
int cimba_tally_reduce_host(const uint32_t* host_rows, uint64_t count,
                            uint32_t K, int device, uint64_t* host_pooled,
                            double* elapsed_ms);
int cimba_gpu_device_count(int* n);
int cimba_gpu_sync(void);
int cimba_scenario_gpu_run(int which, void* result_out);
int cimba_spillprobe_gpu_run(uint64_t ntrials, uint64_t num_objects,
                             uint64_t seed, uint64_t trial_base, int device,
                             double* elapsed_ms, void* results_out);
int cimba_mg1_gpu_run(uint64_t ntrials, const void* params, uint64_t seed,
                      uint64_t trial_base, int device, double* elapsed_ms,
                      void* results_out);
int cimba_jobshop_gpu_run(uint64_t ntrials, const void* params,
                          uint64_t seed, uint64_t trial_base, int device,
                          double* elapsed_ms, void* results_out);
int cimba_sample_gpu(int dist, double p0, uint64_t n, uint64_t seed,
                     int device, double* host_out, double* elapsed_ms,
                     uint32_t blocks);
int cimba_sample_moments_gpu(int dist, double p0, uint64_t n, uint64_t seed,
                             int device, double* out7, double* elapsed_ms);
int cimba_sample_moments_gpu2(int dist, double p0, uint64_t n,
                              uint64_t seed, int device, int use_mfma,
                              double* out7, double* elapsed_ms,
                              uint32_t blocks);
int cimba_awacs_gpu_run(uint64_t ntrials, const void* params, uint64_t seed,
                        uint64_t trial_base, int device, double* elapsed_ms,
                        void* results_out);
int cimba_awacs_power_test(const void* params, uint64_t seed, int device,
                           float* out_powers, int* nt_out);
int cimba_awacs_power_test_devinit(const void* params, uint64_t seed,
                                   int device, float* out_powers,
                                   int* nt_out);
int cimba_awacs_first_dwell_dbg(const void* params, uint64_t master_seed,
                                int device, float* out_powers);
// AWACS per-target / per-stage test entry points (hip/awacs_kernel.hip)
int cimba_awacs_gpu_run_state(uint64_t ntrials, const void* params,
                              uint64_t seed, uint64_t trial_base, int device,
                              int kernel, double* elapsed_ms,
                              void* results_out, void* stores_out);
size_t cimba_awacs_storage_bytes(void);
int cimba_awacs_bf_test(const void* params, uint64_t seed, int device,
                        int devinit, void* st_inout, float* out_powers);
int cimba_awacs_bfidx_test(void* st_inout, const int* idx, int cnt,
                           int nalloc, int mode, int device);
int cimba_awacs_dwell_test(const void* params, void* st_inout, int nwaves,
                           uint32_t trial, uint32_t dwl, float dt, double now,
                           int device);
int cimba_xlane_repro(int iters, int device, int* out64);
int cimba_mm1_multigpu_rccl(uint64_t ntrials, double arr_mean,
                            double srv_mean, uint64_t num_objects,
                            uint64_t seed, int ndev, double* out10);
int cimba_terrain_gpu_build(int cols, int rows, double base, double amp,
                            int octaves, uint64_t seed, int device,
                            void** handle_out);
int cimba_terrain_gpu_stats(void* handle, int cols, int rows, double out4[4]);
int cimba_terrain_gpu_sample(void* handle, int cols, int rows, double base,
                             double amp, int octaves, uint64_t seed,
                             const float* xs, const float* ys, float* out,
                             uint32_t n);
int cimba_terrain_gpu_los(void* handle, int cols, int rows, double base,
                          double amp, int octaves, uint64_t seed,
                          const float* queries, uint8_t* vis, uint32_t nq,
                          int nsteps, double* elapsed_ms);
int cimba_terrain_gpu_free(void* handle);
}

using cmb_models::AWACS;

// Default radar/terrain configuration (BASELINE config 5 with terrain
// masking ON).  The terrain is shared read-only across every trial of a
// run — built once per device / once per host process from a FIXED seed,
// exactly as the reference keeps one terrain per device.
static constexpr int AWACS_TCOLS = 2048, AWACS_TROWS = 2048;
static constexpr uint64_t AWACS_TSEED = 0xC1BA0001ull;

static cmb::TerrainDesc make_awacs_tdesc(double area) {
    cmb::TerrainDesc T;
    T.cols = AWACS_TCOLS;
    T.rows = AWACS_TROWS;
    T.x0 = (float)-area;
    T.y0 = (float)-area;
    T.dx = (float)(2.0 * area / (AWACS_TCOLS - 1));
    T.dy = (float)(2.0 * area / (AWACS_TROWS - 1));
    T.base = 0.0f;
    T.amp = 3000.0f;   // mountainous: real shielding vs a 9 km platform
    T.octaves = 5;
    T.seed = AWACS_TSEED;
    return T;
}

// host-side terrain cache (one heightmap per process; ~16 MB)
static const float* awacs_host_terrain(const cmb::TerrainDesc& T) {
    static std::vector<float> h;
    static bool built = false;
    if (!built) {
        h.resize((size_t)T.cols * T.rows);
        for (int32_t r = 0; r < T.rows; ++r)
            for (int32_t c = 0; c < T.cols; ++c)
                h[(size_t)r * T.cols + c] = cmb::th_texel_height(T, c, r);
        built = true;
    }
    return h.data();
}

static AWACS::Params make_awacs_params(double duration, double dwell,
                                       double maneuver_mean, int ntargets,
                                       double area, double speed,
                                       double snr_ref, int use_terrain) {
    AWACS::Params p;
    p.duration = duration;
    p.dwell = dwell;
    p.maneuver_mean = maneuver_mean;
    p.ntargets = ntargets;
    p.use_terrain = use_terrain;
    p.area = area;
    p.speed = speed;
    p.snr_ref = snr_ref;
    p.sensor_alt = 9000.0;
    p.rot_rate = 0.6283185307179586;  // 6 RPM
    p.beamwidth = 0.0262;             // ~1.5 deg
    p.range_res = 150.0;
    p.cfar_alpha = 3.0;
    p.cfar_nref = 4;
    p.cfar_nguard = 1;
    p.noise_floor = 1.0e-19;
    p.gamma0 = 0.05;
    p.rough_m = 0.03;   // ~lambda/(4 pi sin(graze)): specular band active
    p.wavelength = 0.1;   // S/L-band-ish
    p.target_height = 12.0;
    p.terrain = nullptr;
    p.tdesc = make_awacs_tdesc(area);
    return p;
}

static py::dict awacs_aggregate(const std::vector<AWACS::Result>& res,
                                double elapsed_ms) {
    uint64_t ev = 0, det = 0, dwl = 0, man = 0, ok = 0, illum = 0,
             shld = 0;
    double pw = 0.0, cl = 0.0;
    int32_t bad = 0;
    for (auto& r : res) {
        ev += r.events;
        det += r.detections;
        dwl += r.dwells;
        man += r.maneuvers;
        pw += r.sum_power;
        illum += r.illuminated;
        shld += r.shielded;
        cl += r.sum_clutter;
        if (r.status == 0)
            ++ok;
        else if (!bad)
            bad = r.status;
    }
    py::dict d;
    d["total_events"] = ev;
    d["total_detections"] = det;
    d["total_dwells"] = dwl;
    d["total_maneuvers"] = man;
    d["sum_power"] = pw;
    d["total_illuminated"] = illum;
    d["total_shielded"] = shld;
    d["sum_clutter"] = cl;
    d["trials_ok"] = ok;
    d["first_bad_status"] = bad;
    if (elapsed_ms >= 0) {
        d["elapsed_ms"] = elapsed_ms;
        d["events_per_sec"] =
            elapsed_ms > 0 ? (double)ev / (elapsed_ms * 1e-3) : 0.0;
        d["target_dwells_per_sec"] = elapsed_ms > 0
            ? (double)dwl * 1000.0 / (elapsed_ms * 1e-3)  // nt folded below
            : 0.0;
    }
    return d;
}

static py::dict awacs_host(uint64_t ntrials, double duration, double dwell,
                           double maneuver_mean, int ntargets, uint64_t seed,
                           int threads, uint64_t trial_base, int terrain) {
    // snr_ref: free-space mode keeps the r01 calibration; the clutter
    // pipeline is calibrated so mid-range E_target crosses the CA-CFAR
    // threshold (clutter cells measure ~3e-13) — detection is then a
    // real clutter/terrain discrimination, not a saturated curve
    AWACS::Params p = make_awacs_params(duration, dwell, maneuver_mean,
                                        ntargets, 50000.0, 250.0,
                                        terrain ? 1.0e4 : 2.0e15, terrain);
    if (terrain) p.terrain = awacs_host_terrain(p.tdesc);
    std::vector<AWACS::Result> res(ntrials);
    {
        py::gil_scoped_release nogil;
        run_host<AWACS>(p, seed, ntrials, threads, res.data(), {}, nullptr,
                        trial_base);
    }
    return awacs_aggregate(res, -1.0);
}

static py::dict awacs_gpu(uint64_t ntrials, double duration, double dwell,
                          double maneuver_mean, int ntargets, uint64_t seed,
                          int device, uint64_t trial_base, int terrain) {
    // terrain pointer is filled in by cimba_awacs_gpu_run (device build)
    AWACS::Params p = make_awacs_params(duration, dwell, maneuver_mean,
                                        ntargets, 50000.0, 250.0,
                                        terrain ? 1.0e4 : 2.0e15, terrain);
    std::vector<AWACS::Result> res(ntrials);
    double ms = 0.0;
    int rc;
    {
        py::gil_scoped_release nogil;
        rc = cimba_awacs_gpu_run(ntrials, &p, seed, trial_base, device, &ms,
                                 res.data());
    }
    if (rc != 0) throw std::runtime_error("hip error " + std::to_string(rc));
    return awacs_aggregate(res, ms);
}

using EngAW = Engine<AWACS>;
using StAW = EngAW::Storage;

static void awacs_hip_check(int rc) {
    if (rc != 0) throw std::runtime_error("hip error " + std::to_string(rc));
}

// the test entry points move whole Storage blocks across the language
// boundary as void*: both translation units must agree on the layout
static void awacs_layout_check() {
    if (cimba_awacs_storage_bytes() != sizeof(StAW))
        throw std::runtime_error("AWACS Storage layout mismatch");
}

template <class T>
static py::array_t<T> awacs_arr(const T* src, size_t n) {
    py::array_t<T> a((py::ssize_t)n);
    std::memcpy(a.mutable_data(), src, n * sizeof(T));
    return a;
}

// fp64 raw best-beam power of a target at (x, y): the target_bf formula
// in double on the f32 steering weights
static double awacs_bf_f64(const AWACS::Globals& g, double x, double y) {
    const double s = sin(atan2(y, x));
    double best = 0.0;
    for (int b = 0; b < AWACS::BEAMS; ++b) {
        double re = 0.0, im = 0.0;
        for (int e = 0; e < AWACS::ELEM; ++e) {
            const double ph = 3.14159265358979 * e * s;
            re += cos(ph) * g.wr[e][b] + sin(ph) * g.wi[e][b];
            im += sin(ph) * g.wr[e][b] - cos(ph) * g.wi[e][b];
        }
        const double pw = re * re + im * im;
        best = pw > best ? pw : best;
    }
    return best;
}

// fp64 free-space composition for target t of g
static double awacs_pow_f64(const AWACS::Globals& g, int t, double bf) {
    const double x = g.x[t], y = g.y[t];
    const double r2 = x * x + y * y + 1.0;
    return bf * g.rcs[t] / (r2 * r2);
}

// numerics: device MFMA beamforming vs host f32 scalar and fp64 reference
// for the same (seeded) target set — raw best-beam power bf[t] and the
// composed power, host-initialised and device-initialised engine.  Device
// arrays are MAX_T long so a write past nt is visible; gpu=false returns
// the host side only (the CPU measurement behind the tolerance).
static py::dict awacs_power_check(int ntargets, uint64_t seed, int device,
                                  bool gpu) {
    AWACS::Params p = make_awacs_params(10.0, 0.04, 5.0, ntargets, 50000.0,
                                        250.0, 2.0e15, /*terrain=*/0);
    // host f32 path + fp64 reference on the identical state
    auto st = std::make_unique<StAW>();
    auto eng = std::make_unique<EngAW>(*st);
    eng->init(&p, seed, 0);
    AWACS::setup(*eng);
    const AWACS::Globals& g = eng->globals;
    const int nt = g.nt;
    py::dict d;
    if (gpu) {
        awacs_layout_check();
        constexpr float SENT = -1.0f;
        for (int v = 0; v < 2; ++v) {
            auto dst = std::make_unique<StAW>(*st);
            for (int t = 0; t < AWACS::MAX_T; ++t)
                dst->hot.globals.bf[t] = SENT;
            std::vector<float> pw(AWACS::MAX_T, 0.f);
            awacs_hip_check(cimba_awacs_bf_test(&p, seed, device, v,
                                                dst.get(), pw.data()));
            const AWACS::Globals& dg = dst->hot.globals;
            py::array_t<double> dp((py::ssize_t)nt);
            for (int t = 0; t < nt; ++t)
                dp.mutable_data()[t] = (double)pw[t];
            d[v ? "device_mfma_devinit" : "device_mfma"] = dp;
            d[v ? "device_pow_full_devinit" : "device_pow_full"] =
                awacs_arr(pw.data(), AWACS::MAX_T);
            d[v ? "device_bf_devinit" : "device_bf"] =
                awacs_arr(dg.bf, AWACS::MAX_T);
            d[v ? "device_nt_devinit" : "device_nt"] = (int)dg.nt;
        }
    }
    py::array_t<double> host32((py::ssize_t)nt), host64((py::ssize_t)nt),
        bf64((py::ssize_t)nt);
    py::array_t<float> bf32((py::ssize_t)nt);
    for (int t = 0; t < nt; ++t) {
        const float bf = AWACS::target_bf(g, t);
        bf32.mutable_data()[t] = bf;
        host32.mutable_data()[t] = (double)AWACS::compose_power(g, t, bf);
        const double b64 = awacs_bf_f64(g, g.x[t], g.y[t]);
        bf64.mutable_data()[t] = b64;
        host64.mutable_data()[t] = awacs_pow_f64(g, t, b64);
    }
    d["host_f32"] = host32;
    d["host_f64"] = host64;
    d["host_bf_f32"] = bf32;
    d["bf_f64"] = bf64;
    d["nt"] = nt;
    return d;
}

// beamform_tile_idx on an index list.  State prepared on the host with
// bf[t] = -1 everywhere; mode 0 tiles the list like the wave kernel, mode
// 1 calls it once per entry with cnt = 1 like the block kernel.
static py::dict awacs_bfidx_check(int ntargets, uint64_t seed,
                                  std::vector<int> idx, int mode,
                                  int device) {
    AWACS::Params p = make_awacs_params(10.0, 0.04, 5.0, ntargets, 50000.0,
                                        250.0, 2.0e15, /*terrain=*/0);
    auto st = std::make_unique<StAW>();
    {
        EngAW eng(*st);
        eng.init(&p, seed, 0);
        AWACS::setup(eng);
    }
    AWACS::Globals& g = st->hot.globals;
    const int nt = g.nt;
    if (mode != 0 && mode != 1) throw std::invalid_argument("mode");
    if ((int)idx.size() > AWACS::MAX_T) throw std::invalid_argument("cnt");
    for (int v : idx)
        if (v < 0 || v >= nt) throw std::invalid_argument("idx out of range");
    for (int t = 0; t < AWACS::MAX_T; ++t) g.bf[t] = -1.0f;
    py::array_t<double> bf64((py::ssize_t)nt);
    py::array_t<float> bf32((py::ssize_t)nt);
    for (int t = 0; t < nt; ++t) {
        bf32.mutable_data()[t] = AWACS::target_bf(g, t);
        bf64.mutable_data()[t] = awacs_bf_f64(g, g.x[t], g.y[t]);
    }
    // pad the list with a canary: the first unlisted target (a listed
    // one only when the list covers every target), so that a row taken
    // past cnt lands on a target whose sentinel the test watches
    const int cnt = (int)idx.size();
    std::vector<char> listed(AWACS::MAX_T, 0);
    for (int v : idx) listed[v] = 1;
    int canary = cnt ? idx[0] : 0;
    for (int t = 0; t < nt; ++t)
        if (!listed[t]) {
            canary = t;
            break;
        }
    idx.resize((size_t)cnt + 64, canary);
    awacs_layout_check();
    awacs_hip_check(cimba_awacs_bfidx_test(st.get(), idx.data(), cnt,
                                           (int)idx.size(), mode, device));
    py::dict d;
    d["nt"] = nt;
    d["canary"] = canary;
    d["device_bf"] = awacs_arr(g.bf, AWACS::MAX_T);
    d["host_bf_f32"] = bf32;
    d["bf_f64"] = bf64;
    return d;
}

// ---- fp64 re-statement of the detection pipeline (clutter cell, CFAR
// mean, multipath, energy, pd) on the f32 target state ----
static double awacs_th_sample_f64(const float* h, const cmb::TerrainDesc& T,
                                  double x, double y) {
    double cx = (x - (double)T.x0) / (double)T.dx;
    double cy = (y - (double)T.y0) / (double)T.dy;
    cx = cx < 0.0 ? 0.0 : cx;
    cy = cy < 0.0 ? 0.0 : cy;
    const double mx = (double)(T.cols - 1), my = (double)(T.rows - 1);
    cx = cx > mx ? mx : cx;
    cy = cy > my ? my : cy;
    const double fx = floor(cx), fy = floor(cy);
    const int32_t c0 = (int32_t)fx, r0 = (int32_t)fy;
    const int32_t c1 = c0 + 1 < T.cols ? c0 + 1 : c0;
    const int32_t r1 = r0 + 1 < T.rows ? r0 + 1 : r0;
    const double tx = cx - fx, ty = cy - fy;
    const double v00 = h[(size_t)r0 * T.cols + c0];
    const double v10 = h[(size_t)r0 * T.cols + c1];
    const double v01 = h[(size_t)r1 * T.cols + c0];
    const double v11 = h[(size_t)r1 * T.cols + c1];
    const double a = v00 + (v10 - v00) * tx;
    const double b = v01 + (v11 - v01) * tx;
    return a + (b - a) * ty;
}

static double awacs_clutter_cell_f64(const AWACS::Params& P, double center,
                                     double bdir) {
    const double ke_re = 4.0 / 3.0 * 6371000.0;
    const double dr = P.range_res, bw = P.beamwidth, sa = P.sensor_alt;
    const double dA_unit = (dr * bw) / (double)(AWACS::CL_NR * AWACS::CL_NC);
    const double hi = fmax((double)P.tdesc.base + (double)P.tdesc.amp, 1.0);
    double acc = 0.0;
    for (int s = 0; s < AWACS::CL_NR * AWACS::CL_NC; ++s) {
        const int i = s / AWACS::CL_NC, j = s % AWACS::CL_NC;
        const double tr = ((double)i + 0.5) / (double)AWACS::CL_NR;
        const double R = fmax(1.0, center - 0.5 * dr + tr * dr);
        const double tc = ((double)j + 0.5) / (double)AWACS::CL_NC;
        const double off = -0.5 * bw + tc * bw;
        const double az = bdir + off;
        const double terr = awacs_th_sample_f64(P.terrain, P.tdesc,
                                                R * cos(az), R * sin(az));
        const double h_eff = sa - terr - (R * R) / (2.0 * ke_re);
        if (h_eff <= 0.0) continue;
        const double sin_graze = fmin(1.0, h_eff / R);
        double tt = terr / hi;
        tt = tt < 0.0 ? 0.0 : (tt > 1.0 ? 1.0 : tt);
        const double sigma0 = P.gamma0 * (1.2 - 0.8 * tt) * sin_graze;
        const double ga = exp(-2.7725887 * (off * off) / (bw * bw));
        acc += sigma0 * (ga * ga) * (R * dA_unit) / (R * R * R * R);
    }
    return acc;
}

static double awacs_multipath_f64(const AWACS::Params& P, double tx,
                                  double ty, double ta, double r2d) {
    const double PI = 3.14159265358979;
    const double sa = P.sensor_alt;
    const double t0 = sa / fmax(sa + ta, 1.0);
    double galt = awacs_th_sample_f64(P.terrain, P.tdesc, tx * t0, ty * t0);
    const double hs0 = sa - galt, ht0 = ta - galt;
    if (hs0 <= 1.0 || ht0 <= 1.0) return 1.0;
    const double t1 = hs0 / (hs0 + ht0);
    galt = awacs_th_sample_f64(P.terrain, P.tdesc, tx * t1, ty * t1);
    const double hs = sa - galt, ht = ta - galt;
    if (hs <= 1.0 || ht <= 1.0) return 1.0;
    const double d_dir = sqrt(r2d * r2d + (hs - ht) * (hs - ht));
    const double b1 = sqrt(t1 * r2d * (t1 * r2d) + hs * hs);
    const double b2 =
        sqrt((1.0 - t1) * r2d * ((1.0 - t1) * r2d) + ht * ht);
    const double delta = b1 + b2 - d_dir;
    const double sin_graze = hs / fmax(1.0, b1);
    const double arg = (4.0 * PI * P.rough_m * sin_graze) / P.wavelength;
    const double rho = 0.9 * exp(-arg * arg);
    if (rho < 0.01) return 1.0;
    const double phase = 2.0 * PI * delta / P.wavelength + PI;
    const double one_way = 1.0 + rho * rho + 2.0 * rho * cos(phase);
    return fmax(one_way * one_way, 1.0e-3);
}

struct AwacsF64 {
    double pd, e_c, bf, pow;
};

// fp64 pd of a LOS-clear target t of g (post-kinematics positions)
static AwacsF64 awacs_pd_f64(const AWACS::Params& P, const AWACS::Globals& g,
                             int t, double now) {
    const double x = g.x[t], y = g.y[t];
    const double bdir = fmod(P.rot_rate * now, 2.0 * 3.14159265358979323846);
    const double ta =
        awacs_th_sample_f64(P.terrain, P.tdesc, x, y) + P.target_height;
    const double r2d = sqrt(x * x + y * y);
    AwacsF64 o;
    o.bf = awacs_bf_f64(g, x, y);
    o.pow = awacs_pow_f64(g, t, o.bf);
    o.e_c = awacs_clutter_cell_f64(P, r2d, bdir);
    const double dr = P.range_res;
    double sum = 0.0;
    int used = 0;
    for (int k = P.cfar_nguard + 1; k <= P.cfar_nguard + P.cfar_nref; ++k) {
        const double rlo = r2d - k * dr, rhi = r2d + k * dr;
        if (rlo > dr) {
            sum += awacs_clutter_cell_f64(P, rlo, bdir);
            ++used;
        }
        sum += awacs_clutter_cell_f64(P, rhi, bdir);
        ++used;
    }
    const double mean = used > 0 ? sum / used : 0.0;
    const double thr = P.cfar_alpha * (mean + P.noise_floor);
    const double mp = awacs_multipath_f64(P, x, y, ta, r2d);
    const double dz = P.sensor_alt - ta;
    const double r2 = r2d * r2d + dz * dz;
    const double bfn = o.bf / (double)(AWACS::ELEM * AWACS::ELEM);
    const double e_t =
        P.snr_ref * bfn * bfn * (double)g.rcs[t] * mp / (r2 * r2);
    const double m = (e_t + o.e_c + P.noise_floor) / fmax(thr, 1.0e-30);
    o.pd = 1.0 / (1.0 + exp(-6.0 * (m - 1.0)));
    return o;
}

static py::dict awacs_globals_dict(const AWACS::Globals& g) {
    py::dict d;
    d["x"] = awacs_arr(g.x, AWACS::MAX_T);
    d["y"] = awacs_arr(g.y, AWACS::MAX_T);
    d["vx"] = awacs_arr(g.vx, AWACS::MAX_T);
    d["vy"] = awacs_arr(g.vy, AWACS::MAX_T);
    d["rcs"] = awacs_arr(g.rcs, AWACS::MAX_T);
    d["alt"] = awacs_arr(g.alt, AWACS::MAX_T);
    d["bf"] = awacs_arr(g.bf, AWACS::MAX_T);
    d["det_cnt"] = awacs_arr(g.det_cnt, AWACS::MAX_T);
    d["wr"] = awacs_arr(&g.wr[0][0], AWACS::ELEM * AWACS::BEAMS);
    d["wi"] = awacs_arr(&g.wi[0][0], AWACS::ELEM * AWACS::BEAMS);
    d["nt"] = (int)g.nt;
    d["detections"] = g.detections;
    d["dwells"] = g.dwells;
    d["maneuvers"] = g.maneuvers;
    d["illuminated"] = g.illuminated;
    d["shielded"] = g.shielded;
    d["sum_power"] = g.sum_power;
    d["sum_clutter"] = g.sum_clutter;
    d["last_t"] = g.last_t;
    return d;
}

// One dwell, stage by stage: the unmodified device dwell function on a
// host-built state against AWACS::physics_all on an identical copy.
// mode: wave | free | block1 | block2 | block4 run the device; host |
// host_free return the host side only (pipeline / free-space).
static py::dict awacs_dwell_check(int ntargets, uint64_t seed, double now,
                                  double dt, uint32_t dwl,
                                  const std::string& mode,
                                  py::object beamwidth, int device) {
    int nwaves = 0;
    bool pipeline = true, gpu = true;
    if (mode == "wave") nwaves = 0;
    else if (mode == "free") pipeline = false;
    else if (mode == "block1") nwaves = 1;
    else if (mode == "block2") nwaves = 2;
    else if (mode == "block4") nwaves = 4;
    else if (mode == "host") gpu = false;
    else if (mode == "host_free") { gpu = false; pipeline = false; }
    else throw std::invalid_argument("unknown mode: " + mode);
    constexpr uint32_t TRIAL = 3;
    constexpr float ALT_SENT = -1.0e30f, BF_SENT = -1.0f;

    // state: host engine, terrain on
    AWACS::Params p = make_awacs_params(10.0, 0.04, 5.0, ntargets, 50000.0,
                                        250.0, 1.0e4, /*terrain=*/1);
    if (!beamwidth.is_none()) p.beamwidth = beamwidth.cast<double>();
    p.terrain = awacs_host_terrain(p.tdesc);
    auto st0 = std::make_unique<StAW>();
    {
        EngAW e0(*st0);
        e0.init(&p, seed, TRIAL);
        AWACS::setup(e0);
    }
    AWACS::Globals& g0 = st0->hot.globals;
    const int nt = g0.nt;
    g0.last_t = now - dt;
    g0.dwells = dwl;
    for (int t = 0; t < AWACS::MAX_T; ++t) {
        g0.alt[t] = ALT_SENT;
        g0.bf[t] = BF_SENT;
    }
    // the dwell's parameters: free-space keeps its own snr calibration
    AWACS::Params pp = p;
    if (!pipeline) {
        pp.use_terrain = 0;
        pp.snr_ref = 2.0e15;
    }

    // host dwell on an identical copy
    auto sth = std::make_unique<StAW>(*st0);
    EngAW eh(*sth);
    eh.init(&pp, seed, TRIAL);
    eh.now = now;
    const float fdt = (float)(eh.now - eh.globals.last_t);
    AWACS::physics_all(eh);
    const AWACS::Globals& gh = sth->hot.globals;

    py::dict d;
    d["nt"] = nt;
    d["init"] = awacs_globals_dict(g0);
    d["host"] = awacs_globals_dict(gh);
    if (gpu) {
        awacs_layout_check();
        auto std_ = std::make_unique<StAW>(*st0);
        awacs_hip_check(cimba_awacs_dwell_test(&pp, std_.get(), nwaves, TRIAL,
                                               dwl, fdt, now, device));
        d["dev"] = awacs_globals_dict(std_->hot.globals);
    }

    // host per-target intermediates on the post-kinematics positions
    py::array_t<int> stage((py::ssize_t)nt);
    py::array_t<double> margin((py::ssize_t)nt), pd((py::ssize_t)nt),
        u((py::ssize_t)nt), pd64((py::ssize_t)nt), bf64((py::ssize_t)nt),
        pow64((py::ssize_t)nt);
    py::array_t<float> bf32((py::ssize_t)nt);
    const float bdir = AWACS::beam_dir_at(pp, now);
    const float halfgate =
        0.5f * (float)(pp.beamwidth + pp.rot_rate * pp.dwell);
    double sum_pow64 = 0.0, sum_clut64 = 0.0;
    for (int t = 0; t < nt; ++t) {
        const float x = gh.x[t], y = gh.y[t];
        const float az = atan2f(y, x);
        float dd = az - bdir;
        while (dd > AWACS::PI_) dd -= 2.0f * AWACS::PI_;
        while (dd < -AWACS::PI_) dd += 2.0f * AWACS::PI_;
        margin.mutable_data()[t] = (double)(fabsf(dd) - halfgate);
        u.mutable_data()[t] = AWACS::draw_u01(TRIAL, dwl, (uint32_t)t);
        int stg = 0;
        double pdv = 0.0, pd64v = 0.0, bf64v = 0.0, pow64v = 0.0;
        float bf32v = 0.0f;
        if (!pipeline) {
            stg = 3;
            bf32v = AWACS::target_bf(gh, t);
            const float pw = AWACS::compose_power(gh, t, bf32v);
            const double snr = (double)pw * pp.snr_ref;
            pdv = snr / (1.0 + snr);
            bf64v = awacs_bf_f64(gh, x, y);
            pow64v = awacs_pow_f64(gh, t, bf64v);
            const double snr64 = pow64v * pp.snr_ref;
            pd64v = snr64 / (1.0 + snr64);
            sum_pow64 += pow64v;
        } else if (AWACS::in_beam(az, bdir, halfgate)) {
            const float alt = cmb::th_sample(pp.terrain, pp.tdesc, x, y) +
                              (float)pp.target_height;
            const float r2d = sqrtf(x * x + y * y);
            const float terr_t = alt - (float)pp.target_height;
            if (AWACS::beyond_horizon(r2d, (float)pp.sensor_alt - terr_t,
                                      (float)pp.target_height)) {
                stg = 1;
            } else if (!AWACS::los_clear_fast(pp, x, y, alt,
                                              AWACS::los_steps(pp, r2d))) {
                stg = 2;
            } else {
                stg = 3;
                bf32v = AWACS::target_bf(gh, t);
                const float mp = AWACS::multipath_gain(pp, x, y, alt, r2d);
                const float e_t = AWACS::target_energy(pp, bf32v, gh.rcs[t],
                                                       r2d, alt, mp);
                const float e_c = AWACS::clutter_cell_host(pp, r2d, bdir);
                const float thr = AWACS::cfar_threshold_host(pp, r2d, bdir);
                pdv = (double)AWACS::detect_pd(e_t, e_c,
                                               (float)pp.noise_floor, thr);
                const AwacsF64 r = awacs_pd_f64(pp, gh, t, now);
                pd64v = r.pd;
                bf64v = r.bf;
                pow64v = r.pow;
                sum_pow64 += r.pow;
                sum_clut64 += r.e_c;
            }
        }
        stage.mutable_data()[t] = stg;
        pd.mutable_data()[t] = pdv;
        pd64.mutable_data()[t] = pd64v;
        bf32.mutable_data()[t] = bf32v;
        bf64.mutable_data()[t] = bf64v;
        pow64.mutable_data()[t] = pow64v;
    }
    d["stage"] = stage;
    d["gate_margin"] = margin;
    d["pd"] = pd;
    d["u"] = u;
    d["pd_f64"] = pd64;
    d["host_bf_f32"] = bf32;
    d["bf_f64"] = bf64;
    d["pow_f64"] = pow64;
    d["sum_power_f64"] = sum_pow64;
    d["sum_clutter_f64"] = sum_clut64;
    d["halfgate"] = (double)halfgate;
    d["bdir"] = (double)bdir;
    return d;
}

// ---- whole runs with the per-target end state ----
static int awacs_kernel_id(const std::string& kernel) {
    if (kernel == "block") return 0;
    if (kernel == "wave") return 1;
    if (kernel == "free") return 2;
    throw std::invalid_argument("kernel must be block, wave or free");
}

static py::dict awacs_state_dict(const std::vector<AWACS::Result>& res,
                                 const std::vector<StAW>& stores, int nt,
                                 double ms) {
    py::dict d = awacs_aggregate(res, ms);
    const py::ssize_t n = (py::ssize_t)res.size();
    py::array_t<float> x({n, (py::ssize_t)nt}), y({n, (py::ssize_t)nt}),
        vx({n, (py::ssize_t)nt}), vy({n, (py::ssize_t)nt});
    py::array_t<uint32_t> dc({n, (py::ssize_t)nt});
    py::array_t<uint64_t> det(n);
    for (py::ssize_t i = 0; i < n; ++i) {
        const AWACS::Globals& g = stores[i].hot.globals;
        const size_t b = sizeof(float) * nt;
        std::memcpy(x.mutable_data(i, 0), g.x, b);
        std::memcpy(y.mutable_data(i, 0), g.y, b);
        std::memcpy(vx.mutable_data(i, 0), g.vx, b);
        std::memcpy(vy.mutable_data(i, 0), g.vy, b);
        std::memcpy(dc.mutable_data(i, 0), g.det_cnt, b);
        det.mutable_data()[i] = res[i].detections;
    }
    d["x"] = x;
    d["y"] = y;
    d["vx"] = vx;
    d["vy"] = vy;
    d["det_cnt"] = dc;
    d["detections"] = det;
    return d;
}

static py::dict awacs_gpu_state(uint64_t ntrials, double duration,
                                double dwell, double maneuver_mean,
                                int ntargets, uint64_t seed,
                                const std::string& kernel, int device,
                                uint64_t trial_base) {
    const int kid = awacs_kernel_id(kernel);
    const int terrain = kid != 2;
    if (ntrials == 0 || ntrials > 2048)
        throw std::invalid_argument("ntrials must be in 1..2048");
    AWACS::Params p = make_awacs_params(duration, dwell, maneuver_mean,
                                        ntargets, 50000.0, 250.0,
                                        terrain ? 1.0e4 : 2.0e15, terrain);
    awacs_layout_check();
    std::vector<AWACS::Result> res(ntrials);
    std::vector<StAW> stores(ntrials);
    double ms = 0.0;
    int rc;
    {
        py::gil_scoped_release nogil;
        rc = cimba_awacs_gpu_run_state(ntrials, &p, seed, trial_base, device,
                                       kid, &ms, res.data(), stores.data());
    }
    awacs_hip_check(rc);
    const int nt = ntargets < AWACS::MAX_T ? ntargets : AWACS::MAX_T;
    return awacs_state_dict(res, stores, nt, ms);
}

// the host engine run as run_host does it, keeping each trial's Storage
static py::dict awacs_host_state(uint64_t ntrials, double duration,
                                 double dwell, double maneuver_mean,
                                 int ntargets, uint64_t seed,
                                 const std::string& kernel,
                                 uint64_t trial_base) {
    const int terrain = awacs_kernel_id(kernel) != 2;
    if (ntrials == 0 || ntrials > 2048)
        throw std::invalid_argument("ntrials must be in 1..2048");
    AWACS::Params p = make_awacs_params(duration, dwell, maneuver_mean,
                                        ntargets, 50000.0, 250.0,
                                        terrain ? 1.0e4 : 2.0e15, terrain);
    if (terrain) p.terrain = awacs_host_terrain(p.tdesc);
    std::vector<AWACS::Result> res(ntrials);
    std::vector<StAW> stores(ntrials);
    {
        py::gil_scoped_release nogil;
        for (uint64_t i = 0; i < ntrials; ++i) {
            EngAW eng(stores[i]);
            const uint64_t gt = trial_base + i;
            eng.init(&p, trial_seed(seed, gt), (uint32_t)gt);
            AWACS::setup(eng);
            eng.run(RunLimits{}.until, RunLimits{}.max_events);
            AWACS::finish(eng, res[i]);
        }
    }
    const int nt = ntargets < AWACS::MAX_T ? ntargets : AWACS::MAX_T;
    return awacs_state_dict(res, stores, nt, -1.0);
}

static const std::map<std::string, int> GPU_DISTS = {
    {"u01", cmb::bulk::DIST_U01},
    {"std_normal", cmb::bulk::DIST_STD_NORMAL},
    {"std_exponential", cmb::bulk::DIST_STD_EXPONENTIAL},
    {"std_gamma", cmb::bulk::DIST_GAMMA},
    {"poisson", cmb::bulk::DIST_POISSON},
};

static int gpu_dist_id(const std::string& dist) {
    auto it = GPU_DISTS.find(dist);
    if (it == GPU_DISTS.end())
        throw std::invalid_argument("unknown gpu distribution: " + dist);
    return it->second;
}

static uint32_t checked_blocks(int64_t blocks) {
    if (blocks < 1 || blocks > (int64_t)cmb::bulk::MAX_BLOCKS)
        throw std::invalid_argument(
            "blocks must be in [1, " +
            std::to_string(cmb::bulk::MAX_BLOCKS) + "]");
    return (uint32_t)blocks;
}

static py::dict rng_sample_gpu(const std::string& dist, double p0, uint64_t n,
                               uint64_t seed, int device, int64_t blocks) {
    const int id = gpu_dist_id(dist);
    const uint32_t nb = checked_blocks(blocks);
    py::array_t<double> out((py::ssize_t)n);
    double ms = 0.0;
    int rc;
    {
        py::gil_scoped_release nogil;
        rc = cimba_sample_gpu(id, p0, n, seed, device, out.mutable_data(),
                              &ms, nb);
    }
    if (rc != 0) throw std::runtime_error("hip error " + std::to_string(rc));
    py::dict d;
    d["samples"] = out;
    d["elapsed_ms"] = ms;
    d["gsamples_per_sec"] = ms > 0 ? (double)n / (ms * 1e6) : 0.0;
    return d;
}

static py::dict rng_moments_gpu(const std::string& dist, double p0, uint64_t n,
                                uint64_t seed, int device, int mfma,
                                int64_t blocks) {
    const int id = gpu_dist_id(dist);
    const uint32_t nb = checked_blocks(blocks);
    double o[7];
    double ms = 0.0;
    int rc;
    {
        py::gil_scoped_release nogil;
        rc = cimba_sample_moments_gpu2(id, p0, n, seed, device, mfma, o, &ms,
                                       nb);
    }
    if (rc != 0) throw std::runtime_error("hip error " + std::to_string(rc));
    py::dict d;
    d["n"] = o[0];
    const double mean = o[1] / o[0];
    d["mean"] = mean;
    d["var"] = o[2] / o[0] - mean * mean;
    d["s1"] = o[1];  // raw power sums, as accumulated on the device
    d["s2"] = o[2];
    d["s3"] = o[3];
    d["s4"] = o[4];
    d["min"] = o[5];
    d["max"] = o[6];
    d["elapsed_ms"] = ms;
    d["gsamples_per_sec"] = ms > 0 ? (double)n / (ms * 1e6) : 0.0;
    return d;
}

using cmb_models::JobShop;
using cmb_models::MG1;

static py::dict mg1_aggregate(const std::vector<MG1::Result>& res,
                              double elapsed_ms) {
    uint64_t ev = 0, objs = 0, ok = 0;
    double sys = 0.0, qw = 0.0;
    int32_t bad = 0;
    py::list per_trial;
    for (auto& r : res) {
        ev += r.events;
        objs += r.obj_cnt;
        sys += r.sum_system;
        qw += r.sum_queue;
        if (r.status == 0)
            ++ok;
        else if (!bad)
            bad = r.status;
        per_trial.append(r.obj_cnt ? r.sum_system / (double)r.obj_cnt : 0.0);
    }
    py::dict d;
    d["total_events"] = ev;
    d["total_objects"] = objs;
    d["trials_ok"] = ok;
    d["first_bad_status"] = bad;
    d["avg_system_time"] = objs ? sys / (double)objs : 0.0;
    d["avg_queue_time"] = objs ? qw / (double)objs : 0.0;
    d["per_trial_avg"] = per_trial;
    if (elapsed_ms >= 0) {
        d["elapsed_ms"] = elapsed_ms;
        d["events_per_sec"] =
            elapsed_ms > 0 ? (double)ev / (elapsed_ms * 1e-3) : 0.0;
    }
    return d;
}

static py::dict mg1_host(uint64_t ntrials, uint64_t num_objects,
                         double arr_rate, double srv_mean, double srv_scv,
                         int dist, uint64_t seed, int threads,
                         uint64_t trial_base) {
    MG1::Params p{1.0 / arr_rate, srv_mean, srv_scv, num_objects, dist, 0};
    std::vector<MG1::Result> res(ntrials);
    {
        py::gil_scoped_release nogil;
        run_host<MG1>(p, seed, ntrials, threads, res.data(), {}, nullptr,
                      trial_base);
    }
    return mg1_aggregate(res, -1.0);
}

static py::dict mg1_gpu(uint64_t ntrials, uint64_t num_objects,
                        double arr_rate, double srv_mean, double srv_scv,
                        int dist, uint64_t seed, int device,
                        uint64_t trial_base) {
    MG1::Params p{1.0 / arr_rate, srv_mean, srv_scv, num_objects, dist, 0};
    std::vector<MG1::Result> res(ntrials);
    double ms = 0.0;
    int rc;
    {
        py::gil_scoped_release nogil;
        rc = cimba_mg1_gpu_run(ntrials, &p, seed, trial_base, device, &ms,
                               res.data());
    }
    if (rc != 0) throw std::runtime_error("hip error " + std::to_string(rc));
    return mg1_aggregate(res, ms);
}

static py::dict jobshop_aggregate(const std::vector<JobShop::Result>& res,
                                  double elapsed_ms) {
    uint64_t ev = 0, done = 0, ok = 0;
    double makespan = 0.0;
    double busy[JobShop::NST] = {0, 0, 0};
    int32_t bad = 0;
    for (auto& r : res) {
        ev += r.events;
        done += r.completed;
        makespan += r.makespan;
        for (int s = 0; s < JobShop::NST; ++s) busy[s] += r.busy_time[s];
        if (r.status == 0)
            ++ok;
        else if (!bad)
            bad = r.status;
    }
    py::dict d;
    d["total_events"] = ev;
    d["total_completed"] = done;
    d["trials_ok"] = ok;
    d["first_bad_status"] = bad;
    d["mean_makespan"] = res.empty() ? 0.0 : makespan / (double)res.size();
    py::list ub;
    for (int s = 0; s < JobShop::NST; ++s)
        ub.append(makespan > 0 ? busy[s] / makespan : 0.0);  // mean units busy
    d["mean_units_busy"] = ub;
    if (elapsed_ms >= 0) {
        d["elapsed_ms"] = elapsed_ms;
        d["events_per_sec"] =
            elapsed_ms > 0 ? (double)ev / (elapsed_ms * 1e-3) : 0.0;
    }
    return d;
}

static JobShop::Params make_jobshop_params(uint64_t entities, int njobs,
                                           double think_mean) {
    JobShop::Params p;
    p.total_entities = entities;
    p.think_mean = think_mean;
    p.srv_mean[0] = 1.0;
    p.srv_mean[1] = 0.7;
    p.srv_mean[2] = 1.3;
    p.njobs = njobs;
    p.pad_ = 0;
    return p;
}

static py::dict jobshop_host(uint64_t ntrials, uint64_t entities, int njobs,
                             double think_mean, uint64_t seed, int threads,
                             uint64_t trial_base) {
    JobShop::Params p = make_jobshop_params(entities, njobs, think_mean);
    std::vector<JobShop::Result> res(ntrials);
    {
        py::gil_scoped_release nogil;
        run_host<JobShop>(p, seed, ntrials, threads, res.data(), {}, nullptr,
                          trial_base);
    }
    return jobshop_aggregate(res, -1.0);
}

static py::dict jobshop_gpu(uint64_t ntrials, uint64_t entities, int njobs,
                            double think_mean, uint64_t seed, int device,
                            uint64_t trial_base) {
    JobShop::Params p = make_jobshop_params(entities, njobs, think_mean);
    std::vector<JobShop::Result> res(ntrials);
    double ms = 0.0;
    int rc;
    {
        py::gil_scoped_release nogil;
        rc = cimba_jobshop_gpu_run(ntrials, &p, seed, trial_base, device, &ms,
                                   res.data());
    }
    if (rc != 0) throw std::runtime_error("hip error " + std::to_string(rc));
    return jobshop_aggregate(res, ms);
}

using cmb_models::Scenario;

static py::dict scenario_result_to_dict(const Scenario::Result& r) {
    py::list trace;
    for (int i = 0; i < r.n; ++i)
        trace.append(py::make_tuple(r.ev[i].t, r.ev[i].code));
    py::dict d;
    d["trace"] = trace;
    d["status"] = r.status;
    d["events"] = r.events;
    return d;
}

static py::dict scenario_host(int which) {
    Scenario::Params p{which};
    auto st = std::make_unique<Engine<Scenario>::Storage>();
    auto eng = std::make_unique<Engine<Scenario>>(*st);
    eng->init(&p, 123, 0);
    Scenario::setup(*eng);
    eng->run(1.0e308, 100000);
    Scenario::Result r;
    Scenario::finish(*eng, r);
    return scenario_result_to_dict(r);
}

static py::dict scenario_gpu(int which) {
    Scenario::Result r;
    int rc = cimba_scenario_gpu_run(which, &r);
    if (rc != 0) throw std::runtime_error("hip error " + std::to_string(rc));
    return scenario_result_to_dict(r);
}

// run scenarios through the full executive (hooks + abandon recovery)
static py::dict scenario_run_host(int which, uint64_t ntrials, int threads) {
    Scenario::Params p{which};
    std::vector<Scenario::Result> res(ntrials);
    // hooks fire on worker THREADS: the counters must be atomic
    std::atomic<int> thread_inits{0}, thread_exits{0}, cleanups{0};
    RunHooks hooks;
    hooks.thread_init = [&](int) { ++thread_inits; };
    hooks.thread_exit = [&](int) { ++thread_exits; };
    hooks.trial_cleanup = [&](uint64_t) { ++cleanups; };
    RunReport rep =
        run_host<Scenario>(p, 77, ntrials, threads, res.data(), {}, &hooks);
    py::dict d;
    d["trials"] = rep.trials;
    d["failed"] = rep.failed;
    d["abandoned"] = rep.abandoned;
    d["thread_inits"] = thread_inits.load();
    d["thread_exits"] = thread_exits.load();
    d["cleanups"] = cleanups.load();
    d["first_status"] = ntrials ? res[0].status : 0;
    return d;
}

static py::dict mm1_host(uint64_t ntrials, uint64_t num_objects, double arr_rate,
                         double srv_rate, uint64_t seed, int threads,
                         uint64_t trial_base) {
    MM1::Params p{1.0 / arr_rate, 1.0 / srv_rate, num_objects};
    std::vector<MM1::Result> res(ntrials);
    {
        py::gil_scoped_release nogil;
        run_host<MM1>(p, seed, ntrials, threads, res.data(), {}, nullptr,
                      trial_base);
    }
    uint64_t ev = 0, objs = 0, ok = 0;
    double wait = 0.0;
    int32_t bad = 0;
    py::list per_trial_avg;
    for (auto& r : res) {
        ev += r.events;
        objs += r.obj_cnt;
        wait += r.sum_wait;
        if (r.status == 0)
            ++ok;
        else if (!bad)
            bad = r.status;
        per_trial_avg.append(r.obj_cnt ? r.sum_wait / (double)r.obj_cnt : 0.0);
    }
    py::dict d;
    d["total_events"] = ev;
    d["total_objects"] = objs;
    d["total_wait"] = wait;
    d["trials_ok"] = ok;
    d["first_bad_status"] = bad;
    d["avg_system_time"] = objs ? wait / (double)objs : 0.0;
    d["per_trial_avg"] = per_trial_avg;
    return d;
}

// shared by mm1_gpu and mm1hot1_gpu: same arguments, same result dict
using Mm1GpuRunPt = int (*)(uint64_t, double, double, uint64_t, uint64_t,
                            uint64_t, int, double, uint64_t, Mm1GpuOut*,
                            double*);

template <class Run = Mm1GpuRunPt>
static py::dict mm1_gpu_via(Run run, uint64_t ntrials,
                            uint64_t num_objects, double arr_rate,
                            double srv_rate, uint64_t seed, int device,
                            uint64_t trial_base) {
    Mm1GpuOut o;
    int rc;
    std::vector<double> pt(ntrials);
    {
        py::gil_scoped_release nogil;
        rc = run(ntrials, 1.0 / arr_rate, 1.0 / srv_rate, num_objects, seed,
                 trial_base, device, 1.0e308, UINT64_C(0xFFFFFFFFFFFFFFFF),
                 &o, pt.data());
    }
    if (rc != 0) throw std::runtime_error("hip error " + std::to_string(rc));
    py::dict d;
    d["elapsed_ms"] = o.elapsed_ms;
    d["total_events"] = o.total_events;
    d["total_objects"] = o.total_objs;
    d["total_wait"] = o.total_wait;
    d["trials_ok"] = o.trials_ok;
    d["first_bad_status"] = o.first_bad_status;
    d["avg_system_time"] = o.total_objs ? o.total_wait / (double)o.total_objs : 0.0;
    d["events_per_sec"] =
        o.elapsed_ms > 0 ? (double)o.total_events / (o.elapsed_ms * 1e-3) : 0.0;
    py::list pl;
    for (double v : pt) pl.append(v);
    d["per_trial_avg"] = pl;
    return d;
}

static py::dict mm1_gpu(uint64_t ntrials, uint64_t num_objects, double arr_rate,
                        double srv_rate, uint64_t seed, int device,
                        uint64_t trial_base) {
    return mm1_gpu_via(&cimba_mm1_gpu_run_pt, ntrials, num_objects, arr_rate,
                       srv_rate, seed, device, trial_base);
}

// M/M/1 with a one-entry hot heap tier on the LDS kernel (models/mm1.hpp
// MM1Hot1): the hot/cold boundary test model
static py::dict mm1hot1_gpu(uint64_t ntrials, uint64_t num_objects,
                            double arr_rate, double srv_rate, uint64_t seed,
                            int device, uint64_t trial_base) {
    return mm1_gpu_via(&cimba_mm1hot1_gpu_run_pt, ntrials, num_objects,
                       arr_rate, srv_rate, seed, device, trial_base);
}

// M/M/1 with the queue's length history on (models/mm1.hpp MM1Rec): the
// test model for the cold statistics records.  per_trial_avg holds each
// trial's time-weighted mean queue length; lane_mode 4 = LDS kernel,
// 3 = all-scratch conv kernel
static py::dict mm1rec_gpu(uint64_t ntrials, uint64_t num_objects,
                           double arr_rate, double srv_rate, uint64_t seed,
                           int device, int lane_mode) {
    if (lane_mode != 3 && lane_mode != 4)
        throw std::invalid_argument("lane_mode must be 3 or 4");
    return mm1_gpu_via(
        [lane_mode](uint64_t n, double am, double sm, uint64_t objs,
                    uint64_t sd, uint64_t tb, int dev, double, uint64_t,
                    Mm1GpuOut* o, double* pt) {
            return cimba_mm1rec_gpu_run_pt(n, am, sm, objs, sd, tb, dev,
                                           lane_mode, o, pt);
        },
        ntrials, num_objects, arr_rate, srv_rate, seed, device, 0);
}

static py::dict mm1rec_host(uint64_t ntrials, uint64_t num_objects,
                            double arr_rate, double srv_rate, uint64_t seed,
                            int threads) {
    using cmb_models::MM1Rec;
    MM1Rec::Params p{1.0 / arr_rate, 1.0 / srv_rate, num_objects};
    std::vector<MM1Rec::Result> res(ntrials);
    {
        py::gil_scoped_release nogil;
        run_host<MM1Rec>(p, seed, ntrials, threads, res.data());
    }
    uint64_t ev = 0, ok = 0;
    double sum = 0.0;
    int32_t bad = 0;
    py::list pl;
    for (auto& r : res) {
        ev += r.events;
        sum += r.sum_wait;
        if (r.status == 0)
            ++ok;
        else if (!bad)
            bad = r.status;
        pl.append(r.sum_wait);
    }
    py::dict d;
    d["total_events"] = ev;
    d["total_wait"] = sum;
    d["trials_ok"] = ok;
    d["first_bad_status"] = bad;
    d["per_trial_avg"] = pl;
    return d;
}

// conv_lds_kernel's per-lane plan for "mm1" or "mg1"
static py::dict lds_layout(const std::string& model) {
    uint32_t v[3];
    if (model == "mm1")
        cimba_mm1_lds_layout(v);
    else if (model == "mg1")
        cimba_mg1_lds_layout(v);
    else
        throw std::invalid_argument("model must be mm1 or mg1");
    py::dict d;
    d["hot_bytes"] = v[0];
    d["lane_stride"] = v[1];
    d["waves_per_cu"] = v[2];
    return d;
}

// host-only: pop sequence [(t, pseq, handle), ...] of the seeded heap
// fuzz (include/cimba/heapfuzz.hpp) at hot-tier size `hot`
static py::list hashheap_tier_fuzz(uint64_t seed, uint64_t nops, int hot) {
    if (hot != 0 && hot != 1 && hot != 2 && hot != 4)
        throw std::invalid_argument("hot must be 0, 1, 2 or 4");
    const auto pops = cmb::heap_tier_fuzz_n(seed, nops, hot);
    py::list out;
    for (const auto& p : pops) out.append(py::make_tuple(p.t, p.pseq, p.handle));
    return out;
}

// ---- device log stream: logged M/M/1 (models/mm1_logged.hpp) ------------
using cmb_models::MM1Log;

// one row of the `log_records` structured array: surviving records,
// un-rotated, sorted by (trial, seq); `value` holds the raw u64 bits
struct PyLogRec {
    uint64_t trial;
    uint32_t seq;
    uint32_t pad0_;
    double t;
    uint32_t flags;
    uint16_t code;
    int16_t proc;
    uint8_t vtype;
    uint8_t pad1_[7];
    uint64_t value;
};

// host half of a log window: validates the request, clips it to the run
// and owns the arena the engine (host) or the launcher (GPU) fills
struct LogHostBuf {
    std::vector<LogRec> recs;
    std::vector<uint32_t> emitted;
    LogSink sink = {nullptr, nullptr, 0, 0, 0, 0};
    uint64_t first = 0, count = 0;

    LogHostBuf(uint64_t log_first, uint64_t log_count, uint32_t cap,
               uint32_t mask, uint64_t trial_base, uint64_t ntrials) {
        const LogSink req = {nullptr, nullptr, log_first, log_count, cap, mask};
        const int rc = log_sink_check(&req, trial_base, ntrials);
        if (rc == LOG_ERR_ARENA_TOO_BIG)
            throw py::value_error(
                "log window too large: log_count * log_capacity * 32 bytes "
                "exceeds 1 GiB");
        if (rc)
            throw py::value_error(
                "bad log window: log_capacity must be >= 1 and trial "
                "indices must fit 32 bits");
        log_clip_window(log_first, log_count, trial_base, ntrials, &first,
                        &count);
        if (count == 0) return;
        recs.resize(count * cap);
        emitted.assign(count, 0);
        sink = {recs.data(), emitted.data(), first, count, cap, mask};
    }
    const LogSink* request() const { return count ? &sink : nullptr; }

    void attach_results(py::dict& d) const {
        uint64_t total = 0;
        for (uint32_t n : emitted) total += n < sink.cap ? n : sink.cap;
        py::array_t<PyLogRec> arr((py::ssize_t)total);
        PyLogRec* o = arr.mutable_data();
        for (uint64_t s = 0; s < count; ++s) {
            const uint32_t n = emitted[s];
            const uint32_t kept = n < sink.cap ? n : sink.cap;
            for (uint32_t q = n - kept; q != n; ++q, ++o) {
                const LogRec& r = recs[s * sink.cap + (q % sink.cap)];
                memset((void*)o, 0, sizeof *o);  // padding bytes too
                o->trial = first + s;
                o->seq = r.seq;
                o->t = r.t;
                o->flags = r.flags;
                o->code = r.code;
                o->proc = r.proc;
                o->vtype = r.vtype;
                o->value = r.value;
            }
        }
        py::array_t<uint32_t> em((py::ssize_t)count);
        for (uint64_t s = 0; s < count; ++s) em.mutable_at(s) = emitted[s];
        d["log_records"] = arr;
        d["log_emitted"] = em;
        d["log_first"] = first;
    }
};

static py::dict mm1log_aggregate(const std::vector<MM1Log::Result>& res) {
    uint64_t ev = 0, objs = 0, ok = 0;
    double wait = 0.0;
    int32_t bad = 0;
    py::list per_trial_avg;
    for (auto& r : res) {
        ev += r.events;
        objs += r.obj_cnt;
        wait += r.sum_wait;
        if (r.status == 0)
            ++ok;
        else if (!bad)
            bad = r.status;
        per_trial_avg.append(r.obj_cnt ? r.sum_wait / (double)r.obj_cnt : 0.0);
    }
    py::dict d;
    d["total_events"] = ev;
    d["total_objects"] = objs;
    d["total_wait"] = wait;
    d["trials_ok"] = ok;
    d["first_bad_status"] = bad;
    d["avg_system_time"] = objs ? wait / (double)objs : 0.0;
    d["per_trial_avg"] = per_trial_avg;
    return d;
}

static py::dict mm1log_host(uint64_t ntrials, uint64_t num_objects,
                            double arr_rate, double srv_rate, uint64_t seed,
                            int threads, uint64_t trial_base,
                            uint64_t log_first, uint64_t log_count,
                            uint32_t log_capacity, uint32_t log_mask) {
    LogHostBuf lb(log_first, log_count, log_capacity, log_mask, trial_base,
                  ntrials);
    MM1Log::Params p{1.0 / arr_rate, 1.0 / srv_rate, num_objects};
    std::vector<MM1Log::Result> res(ntrials);
    {
        py::gil_scoped_release nogil;
        run_host<MM1Log>(p, seed, ntrials, threads, res.data(), {}, nullptr,
                         trial_base, lb.request());
    }
    py::dict d = mm1log_aggregate(res);
    lb.attach_results(d);
    return d;
}

static py::dict mm1log_gpu(uint64_t ntrials, uint64_t num_objects,
                           double arr_rate, double srv_rate, uint64_t seed,
                           int device, uint64_t trial_base,
                           const std::string& kernel, uint32_t blocks,
                           uint64_t log_first, uint64_t log_count,
                           uint32_t log_capacity, uint32_t log_mask) {
    static const std::map<std::string, int> KERNELS = {
        {"wave", 0}, {"lane", 1}, {"scratch", 2}, {"conv", 3}};
    const auto kit = KERNELS.find(kernel);
    if (kit == KERNELS.end())
        throw py::value_error("kernel must be wave/lane/scratch/conv, got '" +
                              kernel + "'");
    // validated here, before any device call
    LogHostBuf lb(log_first, log_count, log_capacity, log_mask, trial_base,
                  ntrials);
    std::vector<MM1Log::Result> res(ntrials);
    double elapsed_ms = 0.0;
    int rc;
    {
        py::gil_scoped_release nogil;
        rc = cimba_mm1log_gpu_run(ntrials, 1.0 / arr_rate, 1.0 / srv_rate,
                                  num_objects, seed, trial_base, device,
                                  kit->second, blocks, lb.request(),
                                  &elapsed_ms, res.data());
    }
    if (rc == LOG_ERR_ARENA_TOO_BIG || rc == LOG_ERR_BAD_SINK)
        throw py::value_error("log window refused by the launcher (code " +
                              std::to_string(rc) + ")");
    if (rc != 0) throw std::runtime_error("hip error " + std::to_string(rc));
    py::dict d = mm1log_aggregate(res);
    const uint64_t ev = d["total_events"].cast<uint64_t>();
    d["elapsed_ms"] = elapsed_ms;
    d["events_per_sec"] =
        elapsed_ms > 0 ? (double)ev / (elapsed_ms * 1e-3) : 0.0;
    lb.attach_results(d);
    return d;
}

// ---- device tally stream: tallied M/M/1 (models/mm1_tally.hpp) ----------
using cmb_models::MM1Tally;

// one element of the `tally_summaries` structured array: a TallyHeader
struct PyTallyHdr {
    double n, mean, m2, m3, m4, mn, mx;
    uint64_t nan;
};
static_assert(sizeof(PyTallyHdr) == sizeof(TallyHeader) &&
                  offsetof(PyTallyHdr, mn) == offsetof(DataSummary, mn) &&
                  offsetof(PyTallyHdr, nan) == offsetof(TallyHeader, nan_cnt),
              "PyTallyHdr mirrors TallyHeader");

// host half of a tally window: validates the request, clips it to the run
// and owns the buffers the engine (host) or the launcher (GPU) fills
struct TallyHostBuf {
    int K;
    uint64_t first = 0, count = 0;
    bool per_trial;
    std::vector<TallyHeader> headers;
    std::vector<uint64_t> pooled;
    std::vector<uint32_t> trial_bins;
    TallyRequest req = {{nullptr, 0, 0}, nullptr, nullptr, nullptr, 0.0};

    // tally_count None = every launched trial from tally_first on
    TallyHostBuf(int K_, uint64_t tally_first, const py::object& tally_count,
                 bool per_trial_, uint64_t trial_base, uint64_t ntrials)
        : K(K_), per_trial(per_trial_) {
        uint64_t want_first = tally_first, want_count;
        if (tally_count.is_none())
            tally_clip_window(tally_first, ~UINT64_C(0), trial_base, ntrials,
                              &want_first, &want_count);
        else
            want_count = tally_count.cast<uint64_t>();
        const TallySink want = {nullptr, want_first, want_count};
        const int rc = tally_sink_check(&want, K, trial_base, ntrials);
        if (rc == TALLY_ERR_ARENA_TOO_BIG)
            throw py::value_error(
                "tally window too large: tally_count * K * 3144 bytes "
                "exceeds 1 GiB; pass a smaller tally_count");
        if (rc)
            throw py::value_error(
                "bad tally window: trial indices must fit 32 bits");
        tally_clip_window(want_first, want_count, trial_base, ntrials, &first,
                          &count);
        pooled.assign((size_t)K * TALLY_NBINS, 0);
        if (count == 0) return;
        headers.resize(count * K);
        if (per_trial) trial_bins.resize(count * K * TALLY_NBINS);
        req = {{nullptr, first, count}, headers.data(), pooled.data(),
               per_trial ? trial_bins.data() : nullptr, 0.0};
    }
    TallyRequest* request() { return count ? &req : nullptr; }

    // host engine: run_host filled `arena`; pool the bins here
    void take_arena(const std::vector<TallyRec>& arena) {
        for (size_t r = 0; r < arena.size(); ++r) {
            headers[r].s = arena[r].s;
            headers[r].nan_cnt = arena[r].nan_cnt;
            uint64_t* col = pooled.data() + (r % K) * TALLY_NBINS;
            for (uint32_t b = 0; b < TALLY_NBINS; ++b) col[b] += arena[r].bins[b];
            if (per_trial)
                memcpy(trial_bins.data() + r * TALLY_NBINS, arena[r].bins,
                       sizeof arena[r].bins);
        }
    }

    void attach_results(py::dict& d) const {
        const py::ssize_t c = (py::ssize_t)count;
        py::array_t<PyTallyHdr> sum(std::vector<py::ssize_t>{c, K});
        if (count)
            memcpy((void*)sum.mutable_data(), headers.data(),
                   headers.size() * sizeof(TallyHeader));
        py::array_t<uint64_t> hist(
            std::vector<py::ssize_t>{K, (py::ssize_t)TALLY_NBINS});
        memcpy(hist.mutable_data(), pooled.data(),
               pooled.size() * sizeof(uint64_t));
        d["tally_first"] = first;
        d["tally_summaries"] = sum;
        d["tally_hist"] = hist;
        if (per_trial) {
            py::array_t<uint32_t> th(
                std::vector<py::ssize_t>{c, K, (py::ssize_t)TALLY_NBINS});
            if (count)
                memcpy(th.mutable_data(), trial_bins.data(),
                       trial_bins.size() * sizeof(uint32_t));
            d["tally_trial_hist"] = th;
        }
    }
};

// Aborted trials stay in the pooled histogram and in the summaries as they
// are (what they observed before the abort); `trials_ok` tells the user.
static py::dict mm1tally_host(uint64_t ntrials, uint64_t num_objects,
                              double arr_rate, double srv_rate, uint64_t seed,
                              int threads, uint64_t trial_base,
                              uint64_t tally_first,
                              const py::object& tally_count,
                              bool per_trial_hist) {
    constexpr int K = Engine<MM1Tally>::TALLY_K;
    TallyHostBuf tb(K, tally_first, tally_count, per_trial_hist, trial_base,
                    ntrials);
    MM1Tally::Params p{1.0 / arr_rate, 1.0 / srv_rate, num_objects};
    std::vector<MM1Tally::Result> res(ntrials);
    {
        py::gil_scoped_release nogil;
        std::vector<TallyRec> arena(tb.count * K);  // value-init: zeroed
        const TallySink sink = {arena.data(), tb.first, tb.count};
        run_host<MM1Tally>(p, seed, ntrials, threads, res.data(), {}, nullptr,
                           trial_base, nullptr, tb.count ? &sink : nullptr);
        tb.take_arena(arena);
    }
    py::dict d = mm1log_aggregate(res);
    tb.attach_results(d);
    return d;
}

static py::dict mm1tally_gpu(uint64_t ntrials, uint64_t num_objects,
                             double arr_rate, double srv_rate, uint64_t seed,
                             int device, uint64_t trial_base,
                             const std::string& kernel, uint32_t blocks,
                             uint64_t tally_first,
                             const py::object& tally_count,
                             bool per_trial_hist) {
    static const std::map<std::string, int> KERNELS = {
        {"auto", -1}, {"wave", 0},    {"lane", 1},
        {"scratch", 2}, {"conv", 3}, {"lds", 4}};
    const auto kit = KERNELS.find(kernel);
    if (kit == KERNELS.end())
        throw py::value_error(
            "kernel must be auto/wave/lane/scratch/conv/lds, got '" + kernel +
            "'");
    // auto: mm1_gpu's policy — the LDS kernel for a batch that fills the
    // chip with 64 trials per wave, the wave kernel below that
    const int kind = kit->second >= 0 ? kit->second : ntrials >= 32768 ? 4 : 0;
    // validated here, before any device call
    TallyHostBuf tb(Engine<MM1Tally>::TALLY_K, tally_first, tally_count,
                    per_trial_hist, trial_base, ntrials);
    std::vector<MM1Tally::Result> res(ntrials);
    double elapsed_ms = 0.0;
    int rc;
    {
        py::gil_scoped_release nogil;
        rc = cimba_mm1tally_gpu_run(ntrials, 1.0 / arr_rate, 1.0 / srv_rate,
                                    num_objects, seed, trial_base, device,
                                    kind, blocks, tb.request(),
                                    &elapsed_ms, res.data());
    }
    if (rc == TALLY_ERR_ARENA_TOO_BIG || rc == TALLY_ERR_BAD_SINK)
        throw py::value_error("tally window refused by the launcher (code " +
                              std::to_string(rc) + ")");
    if (rc != 0) throw std::runtime_error("hip error " + std::to_string(rc));
    py::dict d = mm1log_aggregate(res);
    const uint64_t ev = d["total_events"].cast<uint64_t>();
    d["elapsed_ms"] = elapsed_ms;
    d["events_per_sec"] =
        elapsed_ms > 0 ? (double)ev / (elapsed_ms * 1e-3) : 0.0;
    d["tally_reduce_ms"] = tb.req.reduce_ms;
    tb.attach_results(d);
    return d;
}

// test hooks: the bin function (-1 = NaN, which lands in no bin), the
// 771 bin edges (lower edge of every bin, then +inf) and the pooling
// kernel alone on a dense [count, K, 770] array
static py::array_t<int32_t> py_tally_bin(
    py::array_t<double, py::array::c_style | py::array::forcecast> x) {
    py::array_t<int32_t> out(x.size());
    const double* p = x.data();
    int32_t* o = out.mutable_data();
    for (py::ssize_t i = 0; i < x.size(); ++i)
        o[i] = p[i] != p[i] ? -1 : (int32_t)tally_bin(p[i]);
    return out;
}

static py::array_t<double> py_tally_edges() {
    py::array_t<double> out((py::ssize_t)TALLY_NBINS + 1);
    for (uint32_t b = 0; b <= TALLY_NBINS; ++b)
        out.mutable_at(b) = tally_edge(b);
    return out;
}

static py::object py_tally_reduce_gpu(
    py::array_t<uint32_t, py::array::c_style | py::array::forcecast> rows,
    int device, bool timing) {
    if (rows.ndim() != 3 || rows.shape(2) != (py::ssize_t)TALLY_NBINS ||
        rows.shape(1) < 1 || rows.shape(1) > TALLY_MAX_K)
        throw py::value_error("expected a uint32 array [count, K, 770], "
                              "1 <= K <= 8");
    const uint32_t K = (uint32_t)rows.shape(1);
    py::array_t<uint64_t> out(
        std::vector<py::ssize_t>{(py::ssize_t)K, (py::ssize_t)TALLY_NBINS});
    double ms = 0.0;
    int rc;
    {
        py::gil_scoped_release nogil;
        rc = cimba_tally_reduce_host(rows.data(), (uint64_t)rows.shape(0), K,
                                     device, out.mutable_data(), &ms);
    }
    if (rc != 0) throw std::runtime_error("hip error " + std::to_string(rc));
    if (timing) return py::make_tuple(out, ms);
    return std::move(out);
}

// record names per registered model; engine records (proc < 0) carry a
// status word as their code
static const char* devlog_name(const std::string& model, uint16_t code,
                               int16_t proc) {
    if (proc < 0) return status_name((int32_t)code);
    if (model == "mm1log") return MM1Log::log_name(code);
    throw py::value_error("no log names registered for model '" + model + "'");
}

static LogRec devlog_unpack(const PyLogRec& p) {
    LogRec r{};
    r.t = p.t;
    r.value = p.value;
    r.flags = p.flags;
    r.seq = p.seq;
    r.code = p.code;
    r.proc = p.proc;
    r.vtype = p.vtype;
    return r;
}

// one line per record, through the native cmb::log_format
static py::list devlog_format(py::array_t<PyLogRec> records, uint64_t seed,
                              const std::string& model) {
    py::list out;
    const PyLogRec* p = records.data();
    char buf[256];
    for (py::ssize_t i = 0; i < records.size(); ++i) {
        const LogRec r = devlog_unpack(p[i]);
        log_format(buf, sizeof buf, r, (uint32_t)p[i].trial,
                   trial_seed(seed, p[i].trial),
                   devlog_name(model, r.code, r.proc));
        out.append(py::str(buf));
    }
    return out;
}

// print a result's records through the host logger (its current mask and
// stream apply): rebuilds the per-trial rings and walks them with
// cmb::log_replay.  Returns the number of records walked.
static uint64_t devlog_replay(py::array_t<PyLogRec> records,
                              py::array_t<uint32_t> emitted, uint64_t first,
                              uint64_t seed, const std::string& model) {
    const uint64_t count = (uint64_t)emitted.size();
    std::vector<uint32_t> kept(count, 0);
    const PyLogRec* p = records.data();
    for (py::ssize_t i = 0; i < records.size(); ++i) {
        const uint64_t s = p[i].trial - first;
        if (s >= count) throw py::value_error("record outside the window");
        ++kept[s];
    }
    // a ring that overflowed kept exactly `cap` records and one that did
    // not kept all of its own, so the largest survivor count reproduces
    // every ring's rotation
    uint32_t cap = 1;
    for (uint32_t k : kept) cap = k > cap ? k : cap;
    for (uint64_t s = 0; s < count; ++s) {
        const uint32_t n = emitted.at(s);
        if (kept[s] != (n < cap ? n : cap))
            throw py::value_error("log_records do not match log_emitted");
    }
    std::vector<LogRec> arena(count * cap);
    for (py::ssize_t i = 0; i < records.size(); ++i)
        arena[(p[i].trial - first) * cap + (p[i].seq % cap)] =
            devlog_unpack(p[i]);
    return log_replay(
        arena.data(), emitted.data(), first, count, cap,
        [&](uint64_t g) { return trial_seed(seed, g); },
        [&](const LogRec& r) { return devlog_name(model, r.code, r.proc); });
}

static int gpu_device_count() {
    int n = 0;
    (void)cimba_gpu_device_count(&n);
    return n;
}

// ---- RNG sampling for statistical tests -----------------------------------

static py::array_t<double> rng_sample(const std::string& dist,
                                      std::vector<double> a, uint64_t n,
                                      uint64_t seed) {
    py::array_t<double> out((py::ssize_t)n);
    double* o = out.mutable_data();
    Rng r;
    r.seed(seed);
    auto P = [&](size_t i) { return i < a.size() ? a[i] : 0.0; };
    if (dist == "u64") {
        for (uint64_t i = 0; i < n; ++i) o[i] = (double)(r.next() >> 11);
    } else if (dist == "uniform") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.uniform(P(0), P(1));
    } else if (dist == "std_normal") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.std_normal();
    } else if (dist == "normal") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.normal(P(0), P(1));
    } else if (dist == "std_exponential") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.std_exponential();
    } else if (dist == "exponential") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.exponential(P(0));
    } else if (dist == "lognormal") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.lognormal(P(0), P(1));
    } else if (dist == "logistic") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.logistic(P(0), P(1));
    } else if (dist == "cauchy") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.cauchy(P(0), P(1));
    } else if (dist == "rayleigh") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.rayleigh(P(0));
    } else if (dist == "weibull") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.weibull(P(0), P(1));
    } else if (dist == "pareto") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.pareto(P(0), P(1));
    } else if (dist == "triangular") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.triangular(P(0), P(1), P(2));
    } else if (dist == "pert") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.pert(P(0), P(1), P(2));
    } else if (dist == "std_gamma") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.std_gamma(P(0));
    } else if (dist == "gamma") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.gamma(P(0), P(1));
    } else if (dist == "erlang") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.erlang((int64_t)P(0), P(1));
    } else if (dist == "hypoexponential") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.hypoexponential(P(0), P(1));
    } else if (dist == "hyperexponential") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.hyperexponential(P(0), P(1), P(2));
    } else if (dist == "std_beta") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.std_beta(P(0), P(1));
    } else if (dist == "beta") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.beta(P(0), P(1), P(2), P(3));
    } else if (dist == "chisquared") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.chisquared(P(0));
    } else if (dist == "std_t_dist") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.std_t_dist(P(0));
    } else if (dist == "t_dist") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.t_dist(P(0), P(1), P(2));
    } else if (dist == "f_dist") {
        for (uint64_t i = 0; i < n; ++i) o[i] = r.f_dist(P(0), P(1));
    } else if (dist == "bernoulli") {
        for (uint64_t i = 0; i < n; ++i) o[i] = (double)r.bernoulli(P(0));
    } else if (dist == "geometric") {
        for (uint64_t i = 0; i < n; ++i) o[i] = (double)r.geometric(P(0));
    } else if (dist == "poisson") {
        for (uint64_t i = 0; i < n; ++i) o[i] = (double)r.poisson(P(0));
    } else if (dist == "binomial") {
        for (uint64_t i = 0; i < n; ++i) o[i] = (double)r.binomial((int64_t)P(0), P(1));
    } else if (dist == "negative_binomial") {
        for (uint64_t i = 0; i < n; ++i) o[i] = (double)r.negative_binomial(P(0), P(1));
    } else if (dist == "discrete_uniform") {
        for (uint64_t i = 0; i < n; ++i)
            o[i] = (double)r.discrete_uniform((int64_t)P(0), (int64_t)P(1));
    } else if (dist == "dice") {
        for (uint64_t i = 0; i < n; ++i) o[i] = (double)r.dice((int64_t)P(0));
    } else if (dist == "discrete_nonuniform") {
        for (uint64_t i = 0; i < n; ++i)
            o[i] = (double)r.discrete_nonuniform(a.data(), (int64_t)a.size());
    } else if (dist == "alias") {
        std::vector<double> prob(a.size());
        std::vector<int32_t> alias(a.size());
        std::vector<int32_t> scratch(2 * a.size());
        alias_build(a.data(), (int64_t)a.size(), prob.data(), alias.data(),
                    scratch.data());
        AliasTable t{prob.data(), alias.data(), (int64_t)a.size()};
        for (uint64_t i = 0; i < n; ++i) o[i] = (double)t.sample(r);
    } else {
        throw std::invalid_argument("unknown distribution: " + dist);
    }
    return out;
}

// Host reference for the bulk kernels: the same cmb::Rng code, the same
// lane seed and the same interleaved layout (cimba/bulk_rng.hpp), so the
// device output can be compared sample by sample.
static py::array_t<double> rng_sample_lanes(const std::string& dist,
                                            double p0, uint64_t n,
                                            uint64_t seed, uint64_t lanes) {
    const int id = gpu_dist_id(dist);
    if (lanes < 1) throw std::invalid_argument("lanes must be >= 1");
    py::array_t<double> out((py::ssize_t)n);
    double* o = out.mutable_data();
    {
        py::gil_scoped_release nogil;
        for (uint64_t g = 0; g < lanes && g < n; ++g) {
            Rng r;
            r.seed(cmb::bulk::lane_seed(seed, g));
            for (uint64_t i = g; i < n; i += lanes)
                o[i] = cmb::bulk::sample_one(r, id, p0);
        }
    }
    return out;
}

// The ziggurat tables exactly as compiled into host and device code.
static py::dict zig_tables() {
    auto arr = [](const double* p, size_t n) {
        py::array_t<double> a((py::ssize_t)n);
        std::memcpy(a.mutable_data(), p, n * sizeof(double));
        return a;
    };
    namespace z = cmb::zig;
    py::dict d;
    d["NOR_X"] = arr(z::NOR_X, 257);
    d["NOR_F"] = arr(z::NOR_F, 257);
    d["NOR_RATIO"] = arr(z::NOR_RATIO, 256);
    d["EXP_X"] = arr(z::EXP_X, 257);
    d["EXP_F"] = arr(z::EXP_F, 257);
    d["EXP_RATIO"] = arr(z::EXP_RATIO, 256);
    d["NOR_R"] = z::NOR_R;
    d["EXP_R"] = z::EXP_R;
    return d;
}

static uint64_t py_fmix64(uint64_t x) { return fmix64(x); }
static uint64_t py_sfc64_raw(uint64_t seed, uint64_t skip) {
    Rng r;
    r.seed(seed);
    for (uint64_t i = 0; i < skip; ++i) (void)r.next();
    return r.next();
}

// ---- terrain + LOS (reference tut_5_2.cu terrain stack; the host build
// below is the fp32 numerics reference for the GPU kernels) ----

static cmb::TerrainDesc terrain_desc_(int cols, int rows, double base,
                                      double amp, int octaves,
                                      uint64_t seed) {
    return cmb::TerrainDesc{cols,          rows,        0.0f, 0.0f, 1.0f,
                            1.0f,          (float)base, (float)amp,
                            octaves,       seed};
}

static py::dict terrain_host(int cols, int rows, double base, double amp,
                             int octaves, uint64_t seed,
                             std::vector<float> xs, std::vector<float> ys,
                             std::vector<float> queries, int nsteps) {
    const cmb::TerrainDesc T = terrain_desc_(cols, rows, base, amp, octaves,
                                             seed);
    std::vector<float> h((size_t)cols * rows);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c)
            h[(size_t)r * cols + c] = cmb::th_texel_height(T, c, r);
    double s1 = 0, s2 = 0, mn = 1e308, mx = -1e308;
    for (float v : h) {
        const double x = (double)v;
        s1 += x;
        s2 += x * x;
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
    }
    const double n = (double)h.size();
    std::vector<float> samples(xs.size());
    for (size_t i = 0; i < xs.size(); ++i)
        samples[i] = cmb::th_sample(h.data(), T, xs[i], ys[i]);
    std::vector<int> vis(queries.size() / 6);
    for (size_t i = 0; i < vis.size(); ++i) {
        const float* q = &queries[i * 6];
        vis[i] = cmb::th_los_clear(h.data(), T, q[0], q[1], q[2], q[3], q[4],
                                   q[5], nsteps)
                     ? 1
                     : 0;
    }
    py::dict d;
    d["stats"] = std::vector<double>{s1 / n, s2 / n - (s1 / n) * (s1 / n),
                                     mn, mx};
    d["samples"] = samples;
    d["vis"] = vis;
    py::array_t<float> hm({rows, cols});
    std::memcpy(hm.mutable_data(), h.data(), h.size() * sizeof(float));
    d["heights"] = hm;
    return d;
}

static py::dict terrain_gpu(int cols, int rows, double base, double amp,
                            int octaves, uint64_t seed,
                            std::vector<float> xs, std::vector<float> ys,
                            std::vector<float> queries, int nsteps,
                            int device) {
    void* hdl = nullptr;
    int rc = cimba_terrain_gpu_build(cols, rows, base, amp, octaves, seed,
                                     device, &hdl);
    if (rc != 0) throw std::runtime_error("terrain build failed");
    double st[4];
    rc = cimba_terrain_gpu_stats(hdl, cols, rows, st);
    if (rc != 0) throw std::runtime_error("terrain stats failed");
    std::vector<float> samples(xs.size());
    if (!xs.empty()) {
        rc = cimba_terrain_gpu_sample(hdl, cols, rows, base, amp, octaves,
                                      seed, xs.data(), ys.data(),
                                      samples.data(), (uint32_t)xs.size());
        if (rc != 0) throw std::runtime_error("terrain sample failed");
    }
    const uint32_t nq = (uint32_t)(queries.size() / 6);
    std::vector<uint8_t> v8(nq);
    double los_ms = 0.0;
    if (nq) {
        rc = cimba_terrain_gpu_los(hdl, cols, rows, base, amp, octaves, seed,
                                   queries.data(), v8.data(), nq, nsteps,
                                   &los_ms);
        if (rc != 0) throw std::runtime_error("terrain los failed");
    }
    cimba_terrain_gpu_free(hdl);
    std::vector<int> vis(v8.begin(), v8.end());
    py::dict d;
    d["stats"] = std::vector<double>{st[0], st[1], st[2], st[3]};
    d["samples"] = samples;
    d["vis"] = vis;
    d["los_ms"] = los_ms;
    return d;
}

PYBIND11_MODULE(_C, m) {
    m.doc() = "cimba_amd native engine (MI355X / gfx950)";

    m.def("mm1_host", &mm1_host, py::arg("ntrials"), py::arg("num_objects"),
          py::arg("arr_rate") = 0.9, py::arg("srv_rate") = 1.0,
          py::arg("seed") = 0x34f05c64d7ad598fULL, py::arg("threads") = 0,
          py::arg("trial_base") = 0);
    m.def("mm1_gpu", &mm1_gpu, py::arg("ntrials"), py::arg("num_objects"),
          py::arg("arr_rate") = 0.9, py::arg("srv_rate") = 1.0,
          py::arg("seed") = 0x34f05c64d7ad598fULL, py::arg("device") = 0,
          py::arg("trial_base") = 0);
    m.def("mm1hot1_gpu", &mm1hot1_gpu, py::arg("ntrials"),
          py::arg("num_objects"), py::arg("arr_rate") = 0.9,
          py::arg("srv_rate") = 1.0, py::arg("seed") = 0x34f05c64d7ad598fULL,
          py::arg("device") = 0, py::arg("trial_base") = 0);
    m.def("mm1rec_gpu", &mm1rec_gpu, py::arg("ntrials"),
          py::arg("num_objects"), py::arg("arr_rate") = 0.9,
          py::arg("srv_rate") = 1.0, py::arg("seed") = 1,
          py::arg("device") = 0, py::arg("lane_mode") = 4);
    m.def("mm1rec_host", &mm1rec_host, py::arg("ntrials"),
          py::arg("num_objects"), py::arg("arr_rate") = 0.9,
          py::arg("srv_rate") = 1.0, py::arg("seed") = 1,
          py::arg("threads") = 1);
    m.def("lds_layout", &lds_layout, py::arg("model"));
    m.def("hashheap_tier_fuzz", &hashheap_tier_fuzz, py::arg("seed"),
          py::arg("nops"), py::arg("hot"));
    // logged M/M/1: the device log stream's worked model
    PYBIND11_NUMPY_DTYPE(PyLogRec, trial, seq, t, flags, code, proc, vtype,
                         value);
    m.def("mm1log_host", &mm1log_host, py::arg("ntrials"),
          py::arg("num_objects"), py::arg("arr_rate") = 0.9,
          py::arg("srv_rate") = 1.0, py::arg("seed") = 0x34f05c64d7ad598fULL,
          py::arg("threads") = 0, py::arg("trial_base") = 0,
          py::arg("log_first") = 0, py::arg("log_count") = 0,
          py::arg("log_capacity") = 64, py::arg("log_mask") = 0xFFFFFFFFu);
    m.def("mm1log_gpu", &mm1log_gpu, py::arg("ntrials"),
          py::arg("num_objects"), py::arg("arr_rate") = 0.9,
          py::arg("srv_rate") = 1.0, py::arg("seed") = 0x34f05c64d7ad598fULL,
          py::arg("device") = 0, py::arg("trial_base") = 0,
          py::arg("kernel") = "conv", py::arg("blocks") = 0,
          py::arg("log_first") = 0, py::arg("log_count") = 0,
          py::arg("log_capacity") = 64, py::arg("log_mask") = 0xFFFFFFFFu);
    // tallied M/M/1: the device tally stream's worked model
    PYBIND11_NUMPY_DTYPE_EX(PyTallyHdr, n, "n", mean, "mean", m2, "m2", m3,
                            "m3", m4, "m4", mn, "min", mx, "max", nan, "nan");
    m.def("mm1tally_host", &mm1tally_host, py::arg("ntrials"),
          py::arg("num_objects"), py::arg("arr_rate") = 0.9,
          py::arg("srv_rate") = 1.0, py::arg("seed") = 0x34f05c64d7ad598fULL,
          py::arg("threads") = 0, py::arg("trial_base") = 0,
          py::arg("tally_first") = 0, py::arg("tally_count") = py::none(),
          py::arg("per_trial_hist") = false);
    m.def("mm1tally_gpu", &mm1tally_gpu, py::arg("ntrials"),
          py::arg("num_objects"), py::arg("arr_rate") = 0.9,
          py::arg("srv_rate") = 1.0, py::arg("seed") = 0x34f05c64d7ad598fULL,
          py::arg("device") = 0, py::arg("trial_base") = 0,
          py::arg("kernel") = "auto", py::arg("blocks") = 0,
          py::arg("tally_first") = 0, py::arg("tally_count") = py::none(),
          py::arg("per_trial_hist") = false);
    m.def("tally_bin", &py_tally_bin, py::arg("x"));
    m.def("tally_edges", &py_tally_edges);
    m.def("tally_reduce_gpu", &py_tally_reduce_gpu, py::arg("rows"),
          py::arg("device") = 0, py::arg("timing") = false);
    m.attr("TALLY_NBINS") = TALLY_NBINS;
    m.def("devlog_format", &devlog_format, py::arg("records"),
          py::arg("seed"), py::arg("model"));
    m.def("devlog_replay", &devlog_replay, py::arg("records"),
          py::arg("emitted"), py::arg("first"), py::arg("seed"),
          py::arg("model"));
    m.def("mg1_host", &mg1_host, py::arg("ntrials"), py::arg("num_objects"),
          py::arg("arr_rate") = 0.8, py::arg("srv_mean") = 1.0,
          py::arg("srv_scv") = 1.0, py::arg("dist") = 1,
          py::arg("seed") = 0x34f05c64d7ad598fULL, py::arg("threads") = 0,
          py::arg("trial_base") = 0);
    m.def("mg1_gpu", &mg1_gpu, py::arg("ntrials"), py::arg("num_objects"),
          py::arg("arr_rate") = 0.8, py::arg("srv_mean") = 1.0,
          py::arg("srv_scv") = 1.0, py::arg("dist") = 1,
          py::arg("seed") = 0x34f05c64d7ad598fULL, py::arg("device") = 0,
          py::arg("trial_base") = 0);
    m.def("jobshop_host", &jobshop_host, py::arg("ntrials"),
          py::arg("entities") = 10000, py::arg("njobs") = 24,
          py::arg("think_mean") = 0.5, py::arg("seed") = 0x34f05c64d7ad598fULL,
          py::arg("threads") = 0, py::arg("trial_base") = 0);
    m.def("jobshop_gpu", &jobshop_gpu, py::arg("ntrials"),
          py::arg("entities") = 10000, py::arg("njobs") = 24,
          py::arg("think_mean") = 0.5, py::arg("seed") = 0x34f05c64d7ad598fULL,
          py::arg("device") = 0, py::arg("trial_base") = 0);
    m.def("awacs_host", &awacs_host, py::arg("ntrials"),
          py::arg("duration") = 60.0, py::arg("dwell") = 0.04,
          py::arg("maneuver_mean") = 5.0, py::arg("ntargets") = 1000,
          py::arg("seed") = 0x34f05c64d7ad598fULL, py::arg("threads") = 0,
          py::arg("trial_base") = 0, py::arg("terrain") = 1);
    m.def("awacs_gpu", &awacs_gpu, py::arg("ntrials"),
          py::arg("duration") = 60.0, py::arg("dwell") = 0.04,
          py::arg("maneuver_mean") = 5.0, py::arg("ntargets") = 1000,
          py::arg("seed") = 0x34f05c64d7ad598fULL, py::arg("device") = 0,
          py::arg("trial_base") = 0, py::arg("terrain") = 1);
    m.def("xlane_repro", [](int iters, int device) {
        std::vector<int> o(64);
        int rc = cimba_xlane_repro(iters, device, o.data());
        if (rc) throw std::runtime_error("hip " + std::to_string(rc));
        return o;
    }, py::arg("iters") = 4, py::arg("device") = 0);
    m.def("awacs_power_check", &awacs_power_check, py::arg("ntargets") = 1000,
          py::arg("seed") = 42ULL, py::arg("device") = 0,
          py::arg("gpu") = true);
    m.def("awacs_bfidx_check", &awacs_bfidx_check, py::arg("ntargets"),
          py::arg("seed"), py::arg("idx"), py::arg("mode") = 0,
          py::arg("device") = 0);
    m.def("awacs_dwell_check", &awacs_dwell_check, py::arg("ntargets"),
          py::arg("seed"), py::arg("now"), py::arg("dt"), py::arg("dwl"),
          py::arg("mode"), py::arg("beamwidth") = py::none(),
          py::arg("device") = 0);
    m.def("awacs_gpu_state", &awacs_gpu_state, py::arg("ntrials"),
          py::arg("duration") = 60.0, py::arg("dwell") = 0.04,
          py::arg("maneuver_mean") = 5.0, py::arg("ntargets") = 1000,
          py::arg("seed") = 0x34f05c64d7ad598fULL,
          py::arg("kernel") = "block", py::arg("device") = 0,
          py::arg("trial_base") = 0);
    m.def("awacs_host_state", &awacs_host_state, py::arg("ntrials"),
          py::arg("duration") = 60.0, py::arg("dwell") = 0.04,
          py::arg("maneuver_mean") = 5.0, py::arg("ntargets") = 1000,
          py::arg("seed") = 0x34f05c64d7ad598fULL,
          py::arg("kernel") = "block", py::arg("trial_base") = 0);
    m.def("awacs_first_dwell_dbg", [](int ntargets, uint64_t master_seed,
                                      int device) {
        AWACS::Params p = make_awacs_params(10.0, 0.04, 5.0, ntargets,
                                            50000.0, 250.0, 2.0e15,
                                            /*terrain=*/0);
        std::vector<float> dev_pow(AWACS::MAX_T, 0.f);
        int rc = cimba_awacs_first_dwell_dbg(&p, master_seed, device,
                                             dev_pow.data());
        if (rc) throw std::runtime_error("hip " + std::to_string(rc));
        // host reference: trial 0 of the same master seed, first-dwell state
        auto st = std::make_unique<Engine<AWACS>::Storage>();
        auto eng = std::make_unique<Engine<AWACS>>(*st);
        eng->init(&p, trial_seed(master_seed, 0), 0);
        AWACS::setup(*eng);
        py::array_t<double> dev((py::ssize_t)ntargets), h((py::ssize_t)ntargets);
        for (int t = 0; t < ntargets; ++t) {
            dev.mutable_data()[t] = (double)dev_pow[t];
            h.mutable_data()[t] = (double)AWACS::target_power(eng->globals, t);
        }
        py::dict d;
        d["dev"] = dev;
        d["host"] = h;
        d["dbg_snr_ref"] = (double)dev_pow[AWACS::MAX_T - 1];
        d["dbg_trial"] = (double)dev_pow[AWACS::MAX_T - 2];
        d["dbg_dwells"] = (double)dev_pow[AWACS::MAX_T - 3];
        d["dbg_draw0"] = (double)dev_pow[AWACS::MAX_T - 4];
        d["dbg_u01_0"] = (double)dev_pow[AWACS::MAX_T - 5];
        d["dbg_pow_lane0_pre"] = (double)dev_pow[AWACS::MAX_T - 6];
        d["dbg_det_lane0_pre"] = (double)dev_pow[AWACS::MAX_T - 7];
        d["dbg_pow_post"] = (double)dev_pow[AWACS::MAX_T - 8];
        d["dbg_det_post"] = (double)dev_pow[AWACS::MAX_T - 9];
        py::list xs, sazs, wrs, accs;
        for (int l = 0; l < 20; ++l) {
            xs.append((double)dev_pow[400 + l]);
            sazs.append((double)dev_pow[500 + l]);
            wrs.append((double)dev_pow[600 + l]);
            accs.append((double)dev_pow[700 + l]);
        }
        d["x20"] = xs; d["saz20"] = sazs; d["wr20"] = wrs; d["acc20"] = accs;


        // host-side comparison for target 0
        d["host_draw0"] = AWACS::detect_draw(0, 0, 0,
                                             (float)h.data()[0], 2.0e15);
        d["host_u01_0"] = AWACS::draw_u01(0, 0, 0);
        return d;
    }, py::arg("ntargets") = 64, py::arg("master_seed") = 11ULL,
       py::arg("device") = 0);
    m.def("spillprobe_run", [](uint64_t ntrials, uint64_t num_objects,
                               uint64_t seed, int device, bool gpu) {
        using SP = cmb_models::SpillProbe;
        std::vector<SP::Result> res(ntrials);
        int rc = 0;
        double ms = -1.0;
        {
            py::gil_scoped_release nogil;
            if (gpu) {
                rc = cimba_spillprobe_gpu_run(ntrials, num_objects, seed, 0,
                                              device, &ms, res.data());
            } else {
                SP::Params p{num_objects};
                run_host<SP>(p, seed, ntrials, 0, res.data());
            }
        }
        if (rc != 0)
            throw std::runtime_error("hip error " + std::to_string(rc));
        uint64_t ev = 0, ok = 0;
        double wait = 0.0;
        int32_t bad = 0;
        py::list per_trial;
        for (auto& r : res) {
            ev += r.events;
            wait += r.sum_wait;
            if (r.status == 0)
                ++ok;
            else if (!bad)
                bad = r.status;
            per_trial.append(py::make_tuple(r.events, r.sum_wait, r.status));
        }
        py::dict d;
        d["total_events"] = ev;
        d["total_wait"] = wait;
        d["trials_ok"] = ok;
        d["first_bad_status"] = bad;
        d["per_trial"] = per_trial;
        return d;
    }, py::arg("ntrials"), py::arg("num_objects"), py::arg("seed") = 1,
       py::arg("device") = 0, py::arg("gpu") = true);
    m.def("scenario_host", &scenario_host, py::arg("which"));
    m.def("scenario_gpu", &scenario_gpu, py::arg("which"));
    m.def("scenario_run_host", &scenario_run_host, py::arg("which"),
          py::arg("ntrials") = 4, py::arg("threads") = 2);

    // logger controls (reference cmb_logger_flags_on/off)
    m.def("logger_flags_on", &logger_flags_on);
    m.def("logger_flags_off", &logger_flags_off);
    m.def("logger_flags", &logger_flags);
    m.attr("LOG_FATAL") = (uint32_t)LOG_FATAL;
    m.attr("LOG_ERROR") = (uint32_t)LOG_ERROR;
    m.attr("LOG_WARNING") = (uint32_t)LOG_WARNING;
    m.attr("LOG_INFO") = (uint32_t)LOG_INFO;

    py::class_<Dataset>(m, "Dataset")
        .def(py::init<>())
        .def("add", &Dataset::add)
        .def("size", &Dataset::size)
        .def("merge", &Dataset::merge)
        .def("sort", &Dataset::sort)
        .def("median", &Dataset::median)
        .def("quantile", &Dataset::quantile)
        .def("fivenum", [](Dataset& d) {
            double o[5];
            d.fivenum(o);
            return py::make_tuple(o[0], o[1], o[2], o[3], o[4]);
        })
        .def("summarize", &Dataset::summarize)
        .def("histogram", &Dataset::histogram)
        .def("acf", &Dataset::acf)
        .def("pacf", &Dataset::pacf)
        .def("values", [](const Dataset& d) {
            return py::array_t<double>((py::ssize_t)d.size(),
                                       d.values().data());
        });

    py::class_<Timeseries>(m, "Timeseries")
        .def(py::init<>())
        .def("add", &Timeseries::add)
        .def("size", &Timeseries::size)
        .def("summarize", &Timeseries::summarize)
        .def("median", &Timeseries::median);
    m.def("mm1_multigpu_rccl", [](uint64_t ntrials, uint64_t num_objects,
                                  double arr_rate, double srv_rate,
                                  uint64_t seed, int ndev) {
        double o[10];
        int rc = cimba_mm1_multigpu_rccl(ntrials, 1.0 / arr_rate,
                                         1.0 / srv_rate, num_objects, seed,
                                         ndev, o);
        if (rc) throw std::runtime_error("rccl/hip error " +
                                         std::to_string(rc));
        py::dict d;
        d["n"] = o[0];
        d["mean_system_time"] = o[1];
        d["var_system_time"] = o[2];
        d["min"] = o[3];
        d["max"] = o[4];
        d["total_events"] = (uint64_t)o[5];
        d["ndev"] = (int)o[6];
        d["elapsed_ms"] = o[7];
        d["events_per_sec"] = o[7] > 0 ? o[5] * 1000.0 / o[7] : 0.0;
        return d;
    }, py::arg("ntrials"), py::arg("num_objects"), py::arg("arr_rate") = 0.9,
       py::arg("srv_rate") = 1.0, py::arg("seed") = 0x34f05c64d7ad598fULL,
       py::arg("ndev") = -1);
    m.def("gpu_device_count", &gpu_device_count);
    m.def("gpu_sync", []() { return cimba_gpu_sync(); });

    m.def("rng_sample", &rng_sample, py::arg("dist"), py::arg("params"),
          py::arg("n"), py::arg("seed") = 1ULL);
    m.def("rng_sample_gpu", &rng_sample_gpu, py::arg("dist"),
          py::arg("p0") = 0.0, py::arg("n") = 1 << 20, py::arg("seed") = 1ULL,
          py::arg("device") = 0,
          py::arg("blocks") = (int64_t)cmb::bulk::DEFAULT_BLOCKS);
    m.def("rng_moments_gpu", &rng_moments_gpu, py::arg("dist"),
          py::arg("p0") = 0.0, py::arg("n") = 1 << 26, py::arg("seed") = 1ULL,
          py::arg("device") = 0, py::arg("mfma") = 0,
          py::arg("blocks") = (int64_t)cmb::bulk::DEFAULT_BLOCKS);
    m.def("rng_sample_lanes", &rng_sample_lanes, py::arg("dist"),
          py::arg("p0"), py::arg("n"), py::arg("seed"), py::arg("lanes"));
    m.def("zig_tables", &zig_tables);
    m.def("fmix64", &py_fmix64);
    m.def("terrain_host", &terrain_host, py::arg("cols"), py::arg("rows"),
          py::arg("base") = 0.0, py::arg("amp") = 1000.0,
          py::arg("octaves") = 6, py::arg("seed") = 1ULL,
          py::arg("xs") = std::vector<float>{},
          py::arg("ys") = std::vector<float>{},
          py::arg("queries") = std::vector<float>{},
          py::arg("nsteps") = 128);
    m.def("terrain_gpu", &terrain_gpu, py::arg("cols"), py::arg("rows"),
          py::arg("base") = 0.0, py::arg("amp") = 1000.0,
          py::arg("octaves") = 6, py::arg("seed") = 1ULL,
          py::arg("xs") = std::vector<float>{},
          py::arg("ys") = std::vector<float>{},
          py::arg("queries") = std::vector<float>{},
          py::arg("nsteps") = 128, py::arg("device") = 0);
    // seed-replay tooling (reference seed discipline):
    // any trial is reproducible from (master_seed, index)
    m.def("trial_seed", [](uint64_t master, uint64_t idx) {
        return trial_seed(master, idx);
    }, py::arg("master_seed"), py::arg("index"));
    m.def("sfc64_raw", &py_sfc64_raw, py::arg("seed"), py::arg("skip") = 0);
    m.def("engine_sizeof_mm1", []() { return sizeof(Engine<MM1>::Storage); });

    py::class_<DataSummary>(m, "DataSummary")
        .def(py::init([]() {
            DataSummary s;
            s.reset();
            return s;
        }))
        .def("add", &DataSummary::add)
        .def("merge", &DataSummary::merge)
        .def("count", &DataSummary::count)
        .def("mean", [](const DataSummary& s) { return s.mean; })
        .def("minimum", [](const DataSummary& s) { return s.mn; })
        .def("maximum", [](const DataSummary& s) { return s.mx; })
        .def("variance", &DataSummary::variance)
        .def("stddev", &DataSummary::stddev)
        .def("skewness", &DataSummary::skewness)
        .def("kurtosis", &DataSummary::kurtosis)
        .def("raw", [](const DataSummary& s) {
            return py::make_tuple(s.n, s.mean, s.m2, s.m3, s.m4, s.mn, s.mx);
        })
        .def_static("from_raw", [](double n, double mean, double m2, double m3,
                                   double m4, double mn, double mx) {
            DataSummary s;
            s.n = n; s.mean = mean; s.m2 = m2; s.m3 = m3; s.m4 = m4;
            s.mn = mn; s.mx = mx;
            return s;
        });

    py::class_<WtdSummary>(m, "WtdSummary")
        .def(py::init([]() {
            WtdSummary s;
            s.reset();
            return s;
        }))
        .def("add", &WtdSummary::add)
        .def("merge", &WtdSummary::merge)
        .def("mean", [](const WtdSummary& s) { return s.mean; })
        .def("sumw", [](const WtdSummary& s) { return s.sumw; })
        .def("variance", &WtdSummary::variance)
        .def("stddev", &WtdSummary::stddev)
        .def("minimum", [](const WtdSummary& s) { return s.mn; })
        .def("maximum", [](const WtdSummary& s) { return s.mx; })
        .def("skewness", &WtdSummary::skewness)
        .def("kurtosis", &WtdSummary::kurtosis)
        .def("raw", [](const WtdSummary& s) {
            return py::make_tuple(s.n, s.sumw, s.mean, s.m2, s.m3, s.m4,
                                  s.mn, s.mx);
        })
        .def_static("from_raw", [](double n, double sumw, double mean,
                                   double m2, double m3, double m4,
                                   double mn, double mx) {
            WtdSummary s;
            s.n = n; s.sumw = sumw; s.mean = mean; s.m2 = m2; s.m3 = m3;
            s.m4 = m4; s.mn = mn; s.mx = mx;
            return s;
        });
}
