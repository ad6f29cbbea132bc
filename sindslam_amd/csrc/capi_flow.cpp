// C ABI: dense flow stage (include/sind_hip.h).
#include "../../include/sind_hip.h"
#include <cstring>
#include "flow.hpp"

struct sind_flow {
    int device = 0; hipStream_t stream = nullptr; sind::FlowEngine eng;
    DevBuf<uint8_t> g0, g1; DevBuf<float> u, v, f0, f1;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

extern "C" {

int sind_flow_set_max_levels(sind_flow* f, int n) { if (!f || n < 0) return SIND_E_ARG; f->eng.max_levels = n; return SIND_OK; }
int sind_flow_set_coarse_chain(sind_flow* f, int on) { if (!f) return SIND_E_ARG; f->eng.solver.coarse_chain = on != 0; return SIND_OK; }
int sind_flow_set_level_up(sind_flow* f, int on) { if (!f) return SIND_E_ARG; f->eng.solver.level_up = on != 0; return SIND_OK; }
int sind_flow_set_latency_tiles(sind_flow* f, int on) { if (!f) return SIND_E_ARG; f->eng.solver.latency_tiles = on != 0; return SIND_OK; }
int sind_device_count(int* count) { if (!count) return SIND_E_ARG; HIP_TRY(hipGetDeviceCount(count)); return SIND_OK; }

int sind_flow_create(int fw, int fh, int max_batch, int device, sind_flow** out) {
    if (!out || fw < 32 || fh < 32 || max_batch < 1) { sind_set_error("sind_flow_create: bad arguments"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(device));
    sind_flow* f = new sind_flow(); f->device = device;
    HIP_TRY(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&f->ev0)); HIP_TRY(hipEventCreate(&f->ev1));
    int r = f->eng.init(fw, fh, max_batch, f->stream);
    if (r != SIND_OK) { delete f; return r; }
    *out = f; return SIND_OK;
}
int sind_flow_destroy(sind_flow* f) {
    if (!f) return SIND_OK;
    (void)hipSetDevice(f->device);
    if (f->stream) { (void)hipStreamSynchronize(f->stream); (void)hipStreamDestroy(f->stream); }
    if (f->ev0) (void)hipEventDestroy(f->ev0);
    if (f->ev1) (void)hipEventDestroy(f->ev1);
    delete f; return SIND_OK;
}
int sind_flow_levels(sind_flow* f, int* ws, int* hs, int cap) {
    if (!f) return SIND_E_ARG;
    for (int i = 0; i < (int)f->eng.levels.size() && i < cap; i++) { ws[i] = f->eng.levels[i].first; hs[i] = f->eng.levels[i].second; }
    return (int)f->eng.levels.size();
}
static int stage_in(sind_flow* f, const uint8_t* i0, const uint8_t* i1, int B) {
    const size_t n = (size_t)f->eng.fw * f->eng.fh * B;
    SIND_TRY(f->g0.alloc(n)); SIND_TRY(f->g1.alloc(n)); SIND_TRY(f->u.alloc(n)); SIND_TRY(f->v.alloc(n));
    HIP_TRY(hipMemcpyAsync(f->g0.p, i0, n, hipMemcpyHostToDevice, f->stream));
    HIP_TRY(hipMemcpyAsync(f->g1.p, i1, n, hipMemcpyHostToDevice, f->stream));
    return SIND_OK;
}
int sind_flow_deepflow(sind_flow* f, const uint8_t* i0, const uint8_t* i1, int B, float* u, float* v) {
    if (!f || !i0 || !i1 || !u || !v || B < 1 || B > f->eng.maxB) { sind_set_error("sind_flow_deepflow: bad arguments"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(f->device));
    SIND_TRY(stage_in(f, i0, i1, B));
    SIND_TRY(f->eng.deepflow(f->g0.p, f->g1.p, B, f->u.p, f->v.p));
    const size_t n = (size_t)f->eng.fw * f->eng.fh * B;
    HIP_TRY(hipMemcpyAsync(u, f->u.p, n * sizeof(float), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipMemcpyAsync(v, f->v.p, n * sizeof(float), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    return SIND_OK;
}
int sind_flow_refine(sind_flow* f, const uint8_t* i0, const uint8_t* i1, int B, float* u, float* v) {
    if (!f || !i0 || !i1 || !u || !v || B < 1 || B > f->eng.maxB) { sind_set_error("sind_flow_refine: bad arguments"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(f->device));
    SIND_TRY(stage_in(f, i0, i1, B));
    const size_t n = (size_t)f->eng.fw * f->eng.fh * B;
    HIP_TRY(hipMemcpyAsync(f->u.p, u, n * sizeof(float), hipMemcpyHostToDevice, f->stream));
    HIP_TRY(hipMemcpyAsync(f->v.p, v, n * sizeof(float), hipMemcpyHostToDevice, f->stream));
    SIND_TRY(f->eng.refine(f->g0.p, f->g1.p, B, f->u.p, f->v.p));
    HIP_TRY(hipMemcpyAsync(u, f->u.p, n * sizeof(float), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipMemcpyAsync(v, f->v.p, n * sizeof(float), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    return SIND_OK;
}
int sind_flow_varref_f32(sind_flow* f, const float* i0, const float* i1, int w, int h, int B, float* u, float* v,
                         int fp, int sor, float alpha, float delta, float gamma, float omega) {
    if (!f || !i0 || !i1 || !u || !v || B < 1 || B > f->eng.maxB || w < 2 || h < 2 || (size_t)w * h > (size_t)f->eng.fw * f->eng.fh) { sind_set_error("sind_flow_varref_f32: bad arguments"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(f->device));
    const size_t n = (size_t)w * h * B;
    SIND_TRY(f->f0.alloc(n)); SIND_TRY(f->f1.alloc(n)); SIND_TRY(f->u.alloc(n)); SIND_TRY(f->v.alloc(n));
    HIP_TRY(hipMemcpyAsync(f->f0.p, i0, n * sizeof(float), hipMemcpyHostToDevice, f->stream));
    HIP_TRY(hipMemcpyAsync(f->f1.p, i1, n * sizeof(float), hipMemcpyHostToDevice, f->stream));
    HIP_TRY(hipMemcpyAsync(f->u.p, u, n * sizeof(float), hipMemcpyHostToDevice, f->stream));
    HIP_TRY(hipMemcpyAsync(f->v.p, v, n * sizeof(float), hipMemcpyHostToDevice, f->stream));
    sind::VarParams V; V.fixedPointIterations = fp; V.sorIterations = sor; V.alpha = alpha; V.delta = delta; V.gamma = gamma; V.omega = omega;
    SIND_TRY(f->eng.varref_f32(f->f0.p, f->f1.p, w, h, B, f->u.p, f->v.p, V));
    HIP_TRY(hipMemcpyAsync(u, f->u.p, n * sizeof(float), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipMemcpyAsync(v, f->v.p, n * sizeof(float), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    return SIND_OK;
}
int sind_flow_deepflow_dev(sind_flow* f, const uint8_t* i0, const uint8_t* i1, int B, float* u, float* v) {
    if (!f || !i0 || !i1 || !u || !v) { sind_set_error("sind_flow_deepflow_dev: null argument"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(f->device));
    return f->eng.deepflow(i0, i1, B, u, v);
}
int sind_flow_refine_dev(sind_flow* f, const uint8_t* i0, const uint8_t* i1, int B, float* u, float* v) {
    if (!f || !i0 || !i1 || !u || !v) { sind_set_error("sind_flow_refine_dev: null argument"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(f->device));
    return f->eng.refine(i0, i1, B, u, v);
}
int sind_debug_rcp_scan(int device, int exp_lo, int exp_hi, unsigned long long out[3]) {
    if (!out || exp_lo < -100 || exp_hi > 100 || exp_lo > exp_hi) { sind_set_error("sind_debug_rcp_scan: bad arguments"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(device));
    DevBuf<unsigned long long> d; SIND_TRY(d.alloc(3));
    const unsigned long long init[3] = {0, 0, ~0ull};
    HIP_TRY(hipMemcpy(d.p, init, sizeof(init), hipMemcpyHostToDevice));
    SIND_TRY(sind::debug_rcp_scan(nullptr, exp_lo, exp_hi, d.p));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d.p, sizeof(init), hipMemcpyDeviceToHost));
    return SIND_OK;
}
int sind_debug_div_scan(int device, unsigned long long counts[3], int* max_exp, unsigned long long by_exp[124]) {
    if (!counts || !max_exp) { sind_set_error("sind_debug_div_scan: null argument"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(device));
    unsigned long long host[164];
    DevBuf<unsigned long long> d; SIND_TRY(d.alloc(164));
    HIP_TRY(hipMemset(d.p, 0, sizeof(host)));
    SIND_TRY(sind::debug_div_scan(nullptr, d.p));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host, d.p, sizeof(host), hipMemcpyDeviceToHost));
    for (int i = 0; i < 3; i++) counts[i] = host[i];
    *max_exp = host[3] ? (int)host[3] - 200 : -1000;
    if (by_exp) for (int i = 0; i < 124; i++) by_exp[i] = host[4 + i];
    return SIND_OK;
}
int sind_debug_coef_math_scan(int device, int exp_lo, int exp_hi, const float numer[3], unsigned long long out[2]) {
    if (!out || !numer || exp_lo < -96 || exp_hi > 100 || exp_lo > exp_hi) { sind_set_error("sind_debug_coef_math_scan: bad arguments (exponents -96 .. 100)"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(device));
    DevBuf<unsigned long long> d; SIND_TRY(d.alloc(2));
    HIP_TRY(hipMemset(d.p, 0, 2 * sizeof(unsigned long long)));
    SIND_TRY(sind::debug_coef_math_scan(nullptr, exp_lo, exp_hi, numer, d.p));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return SIND_OK;
}

int sind_debug_flow_thresholds(const int* hist, int n, int width, int height, int variant, int device, int* res, double* mu1) {
    if (!hist || !res || n < 1 || variant < 0 || variant > 2 || width < 1 || height < 1) { sind_set_error("sind_debug_flow_thresholds: bad arguments"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(device));
    DevBuf<int> dh, dr; DevBuf<double> dm; SIND_TRY(dh.alloc((size_t)n * 257)); SIND_TRY(dr.alloc((size_t)n * 261)); if (mu1) SIND_TRY(dm.alloc((size_t)n * 256));
    HIP_TRY(hipMemcpy(dh.p, hist, (size_t)n * 257 * sizeof(int), hipMemcpyHostToDevice)); HIP_TRY(hipMemset(dr.p, 0, (size_t)n * 261 * sizeof(int)));
    SIND_TRY(sind::debug_flow_thresholds(nullptr, dh.p, n, width, height, variant, dr.p, mu1 ? dm.p : nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(res, dr.p, (size_t)n * 261 * sizeof(int), hipMemcpyDeviceToHost));
    if (mu1) HIP_TRY(hipMemcpy(mu1, dm.p, (size_t)n * 256 * sizeof(double), hipMemcpyDeviceToHost));
    if (variant == 2) {                                 // the working histograms must have been cleared: hand them back in the first words of every result block
        std::vector<int> back((size_t)n * 257); HIP_TRY(hipMemcpy(back.data(), dh.p, back.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) for (int k = 0; k < 257; k++) res[(size_t)i * 261 + k] = back[(size_t)i * 257 + k];
    }
    return SIND_OK;
}
int sind_debug_large_motion(const float* u, const float* v, int B, int fw, int fh, int W, int H, int device, int* flags, int* hist, float* maxflow, int* end) {
    if (!u || !v || !flags || B < 1 || B > 4096 || fw < 1 || fh < 1 || fw > W || fh > H || W > 16384 || H > 16384) { sind_set_error("sind_debug_large_motion: bad arguments"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(device));
    const int nf = fw * fh; const size_t n = (size_t)nf * B;
    DevBuf<float> du, dv, dmag; DevBuf<unsigned> dmax; DevBuf<int> dh;
    SIND_TRY(du.alloc(n)); SIND_TRY(dv.alloc(n)); SIND_TRY(dmag.alloc(n)); SIND_TRY(dmax.alloc(B)); SIND_TRY(dh.alloc((size_t)B * 256));
    HIP_TRY(hipMemcpy(du.p, u, n * sizeof(float), hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(dv.p, v, n * sizeof(float), hipMemcpyHostToDevice));
    SIND_TRY(sind::launch_mag_stats(nullptr, du.p, dv.p, dmag.p, dmax.p, dh.p, nullptr, nf, B));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<unsigned> h_max(B); std::vector<int> h_hist((size_t)B * 256);
    HIP_TRY(hipMemcpy(h_max.data(), dmax.p, B * sizeof(unsigned), hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(h_hist.data(), dh.p, h_hist.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int b = 0; b < B; b++) {
        float m; std::memcpy(&m, &h_max[b], 4);
        flags[b] = sind::large_motion_decision(m, h_hist.data() + (size_t)b * 256, W, H, end ? end + 2 * b : nullptr) ? 1 : 0;
        if (maxflow) maxflow[b] = m;
    }
    if (hist) std::copy(h_hist.begin(), h_hist.end(), hist);
    return SIND_OK;
}
int sind_debug_flow_masks_batch(const float* u, const float* v, const double* hm, int n, int width, int height, int device,
                                uint8_t* low_batch, uint8_t* high_batch, int* res_batch, uint8_t* low_frame, uint8_t* high_frame, int* res_frame) {
    return sind_debug_flow_masks_stage(u, v, hm, n, width, height, device, low_batch, high_batch, res_batch, low_frame, high_frame, res_frame, 0, nullptr, nullptr, nullptr, nullptr);
}
int sind_debug_flow_masks_stage(const float* u, const float* v, const double* hm, int n, int width, int height, int device,
                                uint8_t* low_batch, uint8_t* high_batch, int* res_batch, uint8_t* low_frame, uint8_t* high_frame, int* res_frame,
                                int byte_offset, float* mag_batch, uint8_t* magu8_batch, float* mag_frame, uint8_t* magu8_frame) {
    if (!u || !v || !hm || !low_batch || !high_batch || !res_batch || !low_frame || !high_frame || !res_frame || n < 1 || n > 64 || width < 64 || width % 64 != 0 || height < 1 || height > 4096 || width > 4096 ||
        byte_offset < 0 || byte_offset > 15) {
        sind_set_error("sind_debug_flow_masks_batch: bad arguments (1..64 frames, width a multiple of 64, byte offset 0..15)"); return SIND_E_ARG;
    }
    HIP_TRY(hipSetDevice(device));
    const size_t np = (size_t)width * height, words = np / 64, slot = sind::flow_mask_slot_words(width, height), res_off = (2 * np + byte_offset + 15) / 16 * 16;
    DevBuf<float> du, dv, dmag; DevBuf<uint8_t> dq, dqf, dmask; DevBuf<int> dh; DevBuf<unsigned long long> dout; DevBuf<sind::FlowMaskRec> drec;
    SIND_TRY(dqf.alloc(np + 16));
    SIND_TRY(du.alloc(np * n)); SIND_TRY(dv.alloc(np * n)); SIND_TRY(dmag.alloc(np * n)); SIND_TRY(dq.alloc(np * n)); SIND_TRY(dh.alloc((size_t)264 * n)); SIND_TRY(dout.alloc(slot * n)); SIND_TRY(drec.alloc(n));
    SIND_TRY(dmask.alloc(res_off + 1088));
    HIP_TRY(hipMemcpy(du.p, u, np * n * sizeof(float), hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(dv.p, v, np * n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dh.p, 0, (size_t)264 * n * sizeof(int))); HIP_TRY(hipMemset(dout.p, 0, slot * n * 8));
    // ---- batched: one record per frame, every frame with workspaces and a working histogram of its own (264 words apart: 16-byte aligned)
    std::vector<sind::FlowMaskRec> recs(n);
    for (int i = 0; i < n; i++) { sind::FlowMaskRec& R = recs[i]; R.U = du.p + np * i; R.V = dv.p + np * i; std::copy(hm + 9 * i, hm + 9 * i + 9, R.H);
                                  R.mag = dmag.p + np * i; R.magu8 = dq.p + np * i; R.hist = dh.p + (size_t)264 * i; R.out = dout.p + slot * i; }
    HIP_TRY(hipMemcpy(drec.p, recs.data(), n * sizeof(sind::FlowMaskRec), hipMemcpyHostToDevice));
    SIND_TRY(sind::launch_flow_masks_frames(nullptr, drec.p, recs.data(), n, n, width, height));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<unsigned long long> out(slot * n);
    HIP_TRY(hipMemcpy(out.data(), dout.p, out.size() * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) {
        const unsigned long long* o = out.data() + slot * i;
        for (size_t k = 0; k < np; k++) { low_batch[np * i + k] = ((o[k >> 6] >> (k & 63)) & 1) ? 128 : 0; high_batch[np * i + k] = ((o[words + (k >> 6)] >> (k & 63)) & 1) ? 255 : 0; }
        std::memcpy(res_batch + (size_t)261 * i, o + 2 * words, 261 * sizeof(int));
    }
    if (mag_batch) HIP_TRY(hipMemcpy(mag_batch, dmag.p, np * n * sizeof(float), hipMemcpyDeviceToHost));
    if (magu8_batch) HIP_TRY(hipMemcpy(magu8_batch, dq.p, np * n, hipMemcpyDeviceToHost));
    // ---- frame by frame: the kernels of DynaTail::flow_masks_gpu (the batched run left every working histogram zeroed; frame 0's serves all).  byte_offset moves the
    // u8 residual and both mask planes off their 16-byte alignment, so that the masks take the one-pixel-per-thread path of k_threshold_masks_dev
    uint8_t* q = dqf.p + byte_offset; uint8_t* low = dmask.p + byte_offset; uint8_t* high = low + np;
    for (int i = 0; i < n; i++) {
        int* res = reinterpret_cast<int*>(dmask.p + res_off);
        SIND_TRY(sind::launch_residual(nullptr, du.p + np * i, dv.p + np * i, hm + 9 * i, dmag.p, reinterpret_cast<unsigned*>(dh.p + 256), dh.p, q, width, height, false));
        SIND_TRY(sind::launch_flow_thresholds_and_masks(nullptr, dh.p, width, height, res, q, low, high));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(low_frame + np * i, low, np, hipMemcpyDeviceToHost)); HIP_TRY(hipMemcpy(high_frame + np * i, high, np, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(res_frame + (size_t)261 * i, res, 261 * sizeof(int), hipMemcpyDeviceToHost));
        if (mag_frame) HIP_TRY(hipMemcpy(mag_frame + np * i, dmag.p, np * sizeof(float), hipMemcpyDeviceToHost));
        if (magu8_frame) HIP_TRY(hipMemcpy(magu8_frame + np * i, q, np, hipMemcpyDeviceToHost));
    }
    return SIND_OK;
}
static bool sor_tiled_ok(int mode, int fuse, int tile_w, int tile_h) {
    const int nt = tile_w * tile_h / 8;
    return (mode == 0 || mode == 4 || mode == 5 || mode == 6) && fuse >= 1 && fuse <= 12 && tile_w >= 16 && tile_w % 8 == 0 && tile_h >= 8 && tile_h % 2 == 0 && nt % 128 == 0 && nt <= 1024 &&
           4 * fuse < tile_w && 4 * fuse < tile_h;
}
int sind_flow_set_sor_tiled(sind_flow* f, int mode, int fuse, int tile_w, int tile_h) {
    if (!f) { sind_set_error("sind_flow_set_sor_tiled: null handle"); return SIND_E_ARG; }
    if (!sor_tiled_ok(mode, fuse, tile_w, tile_h)) { sind_set_error("sind_flow_set_sor_tiled: bad arguments (mode %d, fuse %d, tile %d x %d)", mode, fuse, tile_w, tile_h); return SIND_E_ARG; }
    sind::SolverCfg& C = f->eng.solver; C.mode = mode; C.fuse = fuse; C.tile_w = tile_w; C.tile_h = tile_h; return SIND_OK;
}
int sind_flow_sor_plan(int mode, int fuse, int tile_w, int tile_h, int wave, int stream_min_b, int latency_tiles, int coarse_chain, int w, int h, int B, int total, int* out, int cap) {
    if (!out || cap < 2 || w < 1 || h < 1 || B < 1 || total < 1 || stream_min_b < 1 || !sor_tiled_ok(mode, fuse, tile_w, tile_h)) { sind_set_error("sind_flow_sor_plan: bad arguments"); return SIND_E_ARG; }
    sind::SolverCfg C; C.mode = mode; C.fuse = fuse; C.tile_w = tile_w; C.tile_h = tile_h; C.wave = wave ? 1 : 0; C.stream_min_b = stream_min_b; C.latency_tiles = latency_tiles != 0; C.coarse_chain = coarse_chain != 0;
    sind::SorPlan plan;
    SIND_TRY(sind::sor_plan(w, h, B, total, sind::VarParams().epsilon, C, &plan));
    const int n = (int)plan.iters.size();
    if (cap < 2 + n) { sind_set_error("sind_flow_sor_plan: %d launches, room for %d", n, cap - 2); return SIND_E_ARG; }
    out[0] = (int)plan.kernel; out[1] = n; std::copy(plan.iters.begin(), plan.iters.end(), out + 2);
    return SIND_OK;
}
int sind_flow_set_solver_workgroups(sind_flow* f, int cap) { if (!f || cap < 0) return SIND_E_ARG; f->eng.solver.stream_wg_cap = cap; return SIND_OK; }
int sind_flow_set_wave_solver(sind_flow* f, int on, int target_items, int bands) {
    if (!f || target_items < 0 || bands < 0 || on < 0 || on > 4) return SIND_E_ARG;
    if (on > 1) f->eng.solver.wave_prefetch = std::min(on - 1, 3);       // (experiment: on = 2 / 3 / 4 selects 1 / 2 / 3 rows in flight)
    f->eng.solver.wave = on ? 1 : 0; f->eng.solver.wave_items = target_items > 0 ? target_items : sind::SolverCfg().wave_items; f->eng.solver.wave_bands = bands; return SIND_OK;
}
int sind_flow_wave_layout(int w, int h, int B, int target_items, int bands, int out[4]) {
    if (w < 1 || h < 1 || B < 1 || target_items < 0 || bands < 0 || !out) return SIND_E_ARG;
    sind::sor_wave_layout(w, h, B, target_items > 0 ? target_items : sind::SolverCfg().wave_items, bands, &out[0], &out[1], &out[2], &out[3]); return SIND_OK;
}
int sind_flow_set_wave_pack(sind_flow* f, int group) { if (!f || group < 0) return SIND_E_ARG; f->eng.solver.wave_group = group; return SIND_OK; }
int sind_flow_wave_pack_layout(int w, int h, int B, int target_items, int bands, int group, int out[6]) {
    if (w < 1 || h < 1 || B < 1 || target_items < 0 || bands < 0 || group < 0 || !out) return SIND_E_ARG;
    const sind::SorWavePack L = sind::sor_wave_pack_layout(w, h, B, target_items > 0 ? target_items : sind::SolverCfg().wave_items, bands, group);
    out[0] = L.G; out[1] = L.Pw; out[2] = L.strips; out[3] = L.IW; out[4] = L.bands; out[5] = L.BH; return SIND_OK;
}
int sind_flow_set_coef_kernel(sind_flow* f, int variant) { if (!f || variant < 0 || variant > 3) return SIND_E_ARG; f->eng.solver.coef_kernel = variant == 3 ? 1 : variant; f->eng.solver.coef_xcd = variant == 3 ? 0 : 1; return SIND_OK; }
int sind_flow_set_sor(sind_flow* f, int mode, int fuse, int tile_w) {
    if (tile_w != 64 && tile_w != 128) { sind_set_error("sind_flow_set_sor: bad arguments"); return SIND_E_ARG; }
    return sind_flow_set_sor_tiled(f, mode, fuse, tile_w, 64);
}
int sind_flow_sync(sind_flow* f) { if (!f) return SIND_E_ARG; HIP_TRY(hipStreamSynchronize(f->stream)); return SIND_OK; }
int sind_flow_timer_begin(sind_flow* f) { if (!f) return SIND_E_ARG; HIP_TRY(hipEventRecord(f->ev0, f->stream)); return SIND_OK; }
int sind_flow_timer_end(sind_flow* f, float* ms) {
    if (!f || !ms) return SIND_E_ARG;
    HIP_TRY(hipEventRecord(f->ev1, f->stream)); HIP_TRY(hipEventSynchronize(f->ev1)); HIP_TRY(hipEventElapsedTime(ms, f->ev0, f->ev1));
    return SIND_OK;
}

}  // extern "C"
