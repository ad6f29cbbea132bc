// DynaDetect engine, state-free front: gray + 0.6 resize, dense flow with the large-motion test, up-scale (reference DynaDetect.cc:1386-1392, :1033-1147).
#include <cstring>
#include "dyna.hpp"

namespace sind {

// ======================================================================================================= front
int DynaFront::init(const DynaConfig& c, int maxB_, hipStream_t s) {
    cfg = c; maxB = maxB_; stream = s;
    const float scale_element = 0.6f;                                   // DD:1033
    fw = (int)(scale_element * c.W); fh = (int)(scale_element * c.H);
    SIND_TRY(flow.init(fw, fh, maxB, s));
    const size_t nf = (size_t)fw * fh * maxB;
    SIND_TRY(g0.alloc(nf)); SIND_TRY(g1.alloc(nf)); SIND_TRY(u.alloc(nf)); SIND_TRY(v.alloc(nf)); SIND_TRY(u2.alloc(nf)); SIND_TRY(v2.alloc(nf)); SIND_TRY(mag.alloc(nf));
    SIND_TRY(maxbits.alloc(maxB)); SIND_TRY(hist.alloc((size_t)maxB * 256)); SIND_TRY(idx_dev.alloc(maxB));
    return SIND_OK;
}

int DynaFront::gray_and_min(const uint8_t* bgr, int n, uint8_t* gray, uint8_t* grayMin) {
    const size_t np = (size_t)cfg.W * cfg.H;
    SIND_TRY(launch_bgr2gray(stream, bgr, gray, np * n, false));
    SIND_TRY(launch_resize_u8(stream, gray, grayMin, cfg.W, cfg.H, fw, fh, n, cfg.W, fw, np, (size_t)fw * fh));
    return SIND_OK;
}

int DynaFront::gather(const uint8_t* pool, const int* idx, int B, uint8_t* out) {
    const size_t fb = (size_t)fw * fh;
    if (fb % 16 == 0) return launch_gather_frames(stream, pool, idx, B, out, fb);
    for (int b = 0; b < B; b++) HIP_TRY(hipMemcpyAsync(out + fb * b, pool + fb * idx[b], fb, hipMemcpyDeviceToDevice, stream));
    return SIND_OK;
}

bool large_motion_decision(float maxFlowf, const int* hist256, int W, int H, int* end2) {
    const float scale_element = 0.6f;
    const double maxFlow = maxFlowf;
    const int endFlow = (int)(10.0f * scale_element * 255.0f / maxFlow);
    int endFlow2 = 0; float ratio = 0.0f;
    const float totalpixel = W * H * scale_element * scale_element;
    for (int i = 0; i < 255; ++i) { ratio += (float)hist256[i]; if (ratio > 0.3f * totalpixel) { endFlow2 = i; break; } }
    if (end2) { end2[0] = endFlow; end2[1] = endFlow2; }
    return endFlow2 > endFlow;
}

int DynaFront::dense_flow(const uint8_t* pool, const int* cur, const int* prev1, const int* prev2, int B, float* U, float* V, int* large_motion,
                          float* dbg_du, float* dbg_dv, float* dbg_ru, float* dbg_rv) {
    if (B < 1 || B > maxB) { sind_set_error("dense_flow: batch %d outside [1,%d]", B, maxB); return SIND_E_ARG; }
    const int nf = fw * fh; const size_t nfB = (size_t)nf * B;
    // pass 1: flow(n, n-2) for every pair (DD:1075); with `speculate` the candidates of pass 2 ride along as pairs B .. 2 B - 1
    const bool spec = speculate && 2 * B <= maxB;
    if (spec) {
        std::vector<int> c2(2 * B), p2x(2 * B);
        for (int b = 0; b < B; b++) { c2[b] = c2[B + b] = cur[b]; p2x[b] = prev2[b]; p2x[B + b] = prev1[b]; }
        SIND_TRY(gather(pool, c2.data(), 2 * B, g0.p)); SIND_TRY(gather(pool, p2x.data(), 2 * B, g1.p));
        SIND_TRY(flow.deepflow(g0.p, g1.p, 2 * B, u.p, v.p));
    } else {
        SIND_TRY(gather(pool, cur, B, g0.p)); SIND_TRY(gather(pool, prev2, B, g1.p));
        SIND_TRY(flow.deepflow(g0.p, g1.p, B, u.p, v.p));
    }
    // large-motion test on |flow| (DD:1081-1114): max, u8 normalisation, histogram on the GPU, percentile test here
    SIND_TRY(launch_mag_stats(stream, u.p, v.p, mag.p, maxbits.p, hist.p, nullptr, nf, B));
    std::vector<unsigned> h_max(B); std::vector<int> h_hist((size_t)B * 256);
    HIP_TRY(hipMemcpyAsync(h_max.data(), maxbits.p, B * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(h_hist.data(), hist.p, (size_t)B * 256 * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_TRY(sind_stream_wait(stream));
    std::vector<int> flagged; std::vector<int> lm(B, 0);
    const float scale_element = 0.6f;
    for (int b = 0; b < B; b++) {
        float maxFlowf; std::memcpy(&maxFlowf, &h_max[b], 4);
        if (large_motion_decision(maxFlowf, h_hist.data() + (size_t)b * 256, cfg.W, cfg.H)) { lm[b] = 1; flagged.push_back(b); }
    }
    if (large_motion) std::copy(lm.begin(), lm.end(), large_motion);
    // pass 2: flow(n, n-1) for the flagged pairs only (DD:1121-1131)
    if (!flagged.empty() && spec) {
        for (int b : flagged) {
            HIP_TRY(hipMemcpyAsync(u.p + (size_t)nf * b, u.p + (size_t)nf * (B + b), nf * sizeof(float), hipMemcpyDeviceToDevice, stream));
            HIP_TRY(hipMemcpyAsync(v.p + (size_t)nf * b, v.p + (size_t)nf * (B + b), nf * sizeof(float), hipMemcpyDeviceToDevice, stream));
        }
    } else if (!flagged.empty()) {
        const int B2 = (int)flagged.size();
        std::vector<int> c2(B2), p2(B2);
        for (int k = 0; k < B2; k++) { c2[k] = cur[flagged[k]]; p2[k] = prev1[flagged[k]]; }
        SIND_TRY(gather(pool, c2.data(), B2, g0.p)); SIND_TRY(gather(pool, p2.data(), B2, g1.p));
        SIND_TRY(flow.deepflow(g0.p, g1.p, B2, u2.p, v2.p));
        for (int k = 0; k < B2; k++) {
            HIP_TRY(hipMemcpyAsync(u.p + (size_t)nf * flagged[k], u2.p + (size_t)nf * k, nf * sizeof(float), hipMemcpyDeviceToDevice, stream));
            HIP_TRY(hipMemcpyAsync(v.p + (size_t)nf * flagged[k], v2.p + (size_t)nf * k, nf * sizeof(float), hipMemcpyDeviceToDevice, stream));
        }
    }
    SIND_TRY(launch_scale2(stream, u.p, v.p, -1.0f, nfB));                                   // imgDenseFlow *= -1 (DD:1080, 1129)
    if (dbg_du) { HIP_TRY(hipMemcpyAsync(dbg_du, u.p, nfB * 4, hipMemcpyDeviceToHost, stream)); HIP_TRY(hipMemcpyAsync(dbg_dv, v.p, nfB * 4, hipMemcpyDeviceToHost, stream)); }
    // refinement against the frame actually used (DD:1133-1143)
    std::vector<int> sel(B); for (int b = 0; b < B; b++) sel[b] = lm[b] ? prev1[b] : prev2[b];
    SIND_TRY(gather(pool, cur, B, g0.p)); SIND_TRY(gather(pool, sel.data(), B, g1.p));
    SIND_TRY(flow.refine(g0.p, g1.p, B, u.p, v.p));
    if (dbg_ru) { HIP_TRY(hipMemcpyAsync(dbg_ru, u.p, nfB * 4, hipMemcpyDeviceToHost, stream)); HIP_TRY(hipMemcpyAsync(dbg_rv, v.p, nfB * 4, hipMemcpyDeviceToHost, stream)); }
    // resize to the full frame and undo the 0.6 scale (DD:1144-1147)
    const float inv = 1.0f / scale_element;
    SIND_TRY(launch_resize_f32(stream, u.p, U, fw, fh, cfg.W, cfg.H, B, inv, true));
    SIND_TRY(launch_resize_f32(stream, v.p, V, fw, fh, cfg.W, cfg.H, B, inv, true));
    HIP_TRY(hipGetLastError());
    return SIND_OK;
}

}  // namespace sind
