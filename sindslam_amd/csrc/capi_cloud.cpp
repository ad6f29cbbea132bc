// C ABI: key-frame cloud generation of the mapping consumer (include/sind_hip.h, "sind_cloud_*").
#include <cstring>
#include "../../include/sind_hip.h"
#include <cmath>
#include "cloud.hpp"
#include "host/cloud_filter.hpp"

static_assert(sizeof(sind_cloud_filter_stats) == sizeof(sind::CfStats) && sizeof(sind_cloud_point) == sizeof(sind::CloudPoint), "the ABI structs are the kernels' structs");

struct sind_cloud {
    int device = 0, W = 0, H = 0, maxB = 0, np = 0, nchunks = 0; sind::CloudCam cam{}; hipStream_t stream = nullptr;
    DevBuf<uint8_t> bgr, dyna, dynaLast, label; DevBuf<uint16_t> depth, depthLast; DevBuf<sind::CloudPose> pose;
    DevBuf<int> chunkCnt, chunkOff, occ, labelCount, kept, total; DevBuf<sind::CloudPoint> out;
    std::vector<sind::CloudPose> h_pose; std::vector<int> h_total;
    int lastB = 0;                                                    // clouds that the last sind_cloud_generate left in `out` (h_total holds their sizes)
    // sind_cloud_filter_outliers: allocated at the first filter call, then reused
    bool filterReady = false;
    DevBuf<sind::CloudPoint> fin, fout; DevBuf<int> fn, fnfin, fcellStart, fcursor, flist, flistN, fchunkOff, fnOut; DevBuf<unsigned> fbbox; DevBuf<sind::CfPlan> fplan;
    DevBuf<float4> fsorted; DevBuf<float> fdist; DevBuf<sind::CfStats> fstats; std::vector<int> h_nout;
    int filter_alloc() {
        if (filterReady) return SIND_OK;
        const size_t B = maxB, n = np; int r = SIND_OK;
        if ((r = fin.alloc(B * n)) || (r = fout.alloc(B * n)) || (r = fn.alloc(B)) || (r = fnfin.alloc(B)) || (r = fcellStart.alloc(B * (sind::CF_CELLS + 1))) || (r = fcursor.alloc(B * sind::CF_CELLS)) ||
            (r = flist.alloc(B * n)) || (r = flistN.alloc(B)) || (r = fchunkOff.alloc(B * divup(np, 1024))) || (r = fnOut.alloc(B)) || (r = fbbox.alloc(B * 6)) || (r = fplan.alloc(B)) ||
            (r = fsorted.alloc(B * n)) || (r = fdist.alloc(B * n)) || (r = fstats.alloc(B))) return r;
        h_nout.resize(B); filterReady = true; return SIND_OK;
    }
};

sind::CloudResident sind::cloud_resident(const sind_cloud* c) { return sind::CloudResident{c->out.p, c->np, c->lastB, c->device, c->h_total.data()}; }

extern "C" {

int sind_cloud_create(double fx, double fy, double cx, double cy, double depth_scale, int width, int height, int max_batch, int device, sind_cloud** out) {
    if (!out || width < 2 || height < 2 || max_batch < 1 || !(fx > 0) || !(fy > 0) || !(depth_scale > 0)) { sind_set_error("sind_cloud_create: bad arguments"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(device));
    sind_cloud* c = new sind_cloud(); c->device = device; c->W = width; c->H = height; c->maxB = max_batch; c->cam = {fx, fy, cx, cy, depth_scale};
    c->np = sind::cloud_grid_points(width, height); c->nchunks = divup(c->np, sind::CLOUD_CHUNK);
    const size_t B = max_batch, px = (size_t)width * height;
    int r = SIND_OK;
    if ((r = c->bgr.alloc(B * px * 3)) || (r = c->dyna.alloc(B * px)) || (r = c->dynaLast.alloc(B * px)) || (r = c->label.alloc(B * px)) || (r = c->depth.alloc(B * px)) ||
        (r = c->depthLast.alloc(B * px)) || (r = c->pose.alloc(B)) || (r = c->chunkCnt.alloc(B * c->nchunks * sind::CLOUD_LABELS)) || (r = c->chunkOff.alloc(B * c->nchunks * sind::CLOUD_LABELS)) ||
        (r = c->occ.alloc(B * sind::CLOUD_LABELS)) || (r = c->labelCount.alloc(B * sind::CLOUD_LABELS)) || (r = c->kept.alloc(B * sind::CLOUD_LABELS)) || (r = c->total.alloc(B)) ||
        (r = c->out.alloc(B * c->np))) { delete c; return r; }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; sind_set_error("sind_cloud_create: stream creation failed"); return SIND_E_HIP; }
    c->h_pose.resize(B); c->h_total.resize(B);
    *out = c; return SIND_OK;
}
int sind_cloud_destroy(sind_cloud* c) {
    if (!c) return SIND_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    hipStream_t s = c->stream; delete c; if (s) (void)hipStreamDestroy(s);
    return SIND_OK;
}
int sind_cloud_max_points(sind_cloud* c) { return c ? c->np : SIND_E_ARG; }

int sind_cloud_generate(sind_cloud* c, int B, const uint8_t* bgr, const uint16_t* depth, const uint16_t* depth_last, const uint8_t* dyna, const uint8_t* dyna_last,
                        const uint8_t* label, const double* pose_relative, const double* Twc, int inputs_on_device, sind_cloud_point* points, int cap, int* n_points,
                        int* occlusion, int* label_count, int* kept) {
    if (!c || B < 1 || B > c->maxB || !bgr || !depth || !depth_last || !dyna || !dyna_last || !label || !pose_relative || !Twc || !n_points || (points && cap < 1)) {
        sind_set_error("sind_cloud_generate: bad arguments (B=%d, max %d)", B, c ? c->maxB : 0); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream; const size_t px = (size_t)c->W * c->H;
    for (int b = 0; b < B; b++) { std::memcpy(c->h_pose[b].rel, pose_relative + 16 * b, 12 * sizeof(double)); std::memcpy(c->h_pose[b].twc, Twc + 16 * b, 12 * sizeof(double)); }
    HIP_TRY(hipMemcpyAsync(c->pose.p, c->h_pose.data(), (size_t)B * sizeof(sind::CloudPose), hipMemcpyHostToDevice, s));
    sind::CloudArrays a{};
    if (inputs_on_device) { a.bgr = bgr; a.depth = depth; a.depthLast = depth_last; a.dyna = dyna; a.dynaLast = dyna_last; a.label = label; }
    else {
        HIP_TRY(hipMemcpyAsync(c->bgr.p, bgr, B * px * 3, hipMemcpyHostToDevice, s)); HIP_TRY(hipMemcpyAsync(c->depth.p, depth, B * px * 2, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(c->depthLast.p, depth_last, B * px * 2, hipMemcpyHostToDevice, s)); HIP_TRY(hipMemcpyAsync(c->dyna.p, dyna, B * px, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(c->dynaLast.p, dyna_last, B * px, hipMemcpyHostToDevice, s)); HIP_TRY(hipMemcpyAsync(c->label.p, label, B * px, hipMemcpyHostToDevice, s));
        a.bgr = c->bgr.p; a.depth = c->depth.p; a.depthLast = c->depthLast.p; a.dyna = c->dyna.p; a.dynaLast = c->dynaLast.p; a.label = c->label.p;
    }
    a.pose = c->pose.p; a.chunkCnt = c->chunkCnt.p; a.chunkOff = c->chunkOff.p; a.occlusion = c->occ.p; a.labelCount = c->labelCount.p; a.kept = c->kept.p; a.total = c->total.p; a.out = c->out.p;
    SIND_TRY(sind::launch_cloud(c->cam, a, c->W, c->H, B, s));
    HIP_TRY(hipMemcpyAsync(c->h_total.data(), c->total.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
    if (occlusion) HIP_TRY(hipMemcpyAsync(occlusion, c->occ.p, (size_t)B * sind::CLOUD_LABELS * sizeof(int), hipMemcpyDeviceToHost, s));
    if (label_count) HIP_TRY(hipMemcpyAsync(label_count, c->labelCount.p, (size_t)B * sind::CLOUD_LABELS * sizeof(int), hipMemcpyDeviceToHost, s));
    if (kept) HIP_TRY(hipMemcpyAsync(kept, c->kept.p, (size_t)B * sind::CLOUD_LABELS * sizeof(int), hipMemcpyDeviceToHost, s));
    c->lastB = 0;
    HIP_TRY(hipStreamSynchronize(s));
    c->lastB = B;
    for (int b = 0; b < B; b++) {
        n_points[b] = c->h_total[b];
        if (!points) continue;
        if (c->h_total[b] > cap) { sind_set_error("sind_cloud_generate: frame %d has %d points, capacity %d", b, c->h_total[b], cap); return SIND_E_CAPACITY; }
        HIP_TRY(hipMemcpyAsync(points + (size_t)b * cap, c->out.p + (size_t)b * c->np, (size_t)c->h_total[b] * sizeof(sind::CloudPoint), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return SIND_OK;
}

int sind_cloud_filter_max_mean_k(void) { return sind::CF_MAX_MEAN_K; }

int sind_cloud_filter_outliers(sind_cloud* c, int B, const sind_cloud_point* points, int stride, const int* n_points, int inputs_on_device, int mean_k, double stddev_mul,
                               sind_cloud_point* out, int out_cap, int* n_out, float* distances, sind_cloud_filter_stats* stats) {
    if (!c || B < 1 || B > c->maxB || !n_out || (points && (!n_points || stride < 1)) || (out && out_cap < 1) || (distances && stride < 1)) {
        sind_set_error("sind_cloud_filter_outliers: bad arguments (B=%d, max %d)", B, c ? c->maxB : 0); return SIND_E_ARG; }
    if (mean_k < 1 || mean_k > sind::CF_MAX_MEAN_K) { sind_set_error("sind_cloud_filter_outliers: mean_k %d outside 1..%d", mean_k, sind::CF_MAX_MEAN_K); return SIND_E_ARG; }
    if (!std::isfinite(stddev_mul)) { sind_set_error("sind_cloud_filter_outliers: stddev_mul is not finite"); return SIND_E_ARG; }
    if (!points && B > c->lastB) { sind_set_error("sind_cloud_filter_outliers: points == NULL asks for %d clouds, the last sind_cloud_generate left %d", B, c->lastB); return SIND_E_STATE; }
    const int* hn = points ? n_points : c->h_total.data();
    int nmax = 0;
    for (int b = 0; b < B; b++) {
        if (hn[b] < 0 || (points && hn[b] > stride)) { sind_set_error("sind_cloud_filter_outliers: cloud %d has n_points %d (stride %d)", b, hn[b], stride); return SIND_E_ARG; }
        if (hn[b] > c->np) { sind_set_error("sind_cloud_filter_outliers: cloud %d has %d points, the handle holds %d", b, hn[b], c->np); return SIND_E_CAPACITY; }
        if (distances && hn[b] > stride) { sind_set_error("sind_cloud_filter_outliers: cloud %d has %d points, distances rows hold %d", b, hn[b], stride); return SIND_E_ARG; }
        nmax = std::max(nmax, hn[b]);
    }
    HIP_TRY(hipSetDevice(c->device));
    SIND_TRY(c->filter_alloc());
    hipStream_t s = c->stream;
    sind::CfArrays a{};
    a.np = c->np;
    if (!points) { a.pts = c->out.p; a.stride = c->np; a.n = c->total.p; }
    else {
        HIP_TRY(hipMemcpyAsync(c->fn.p, n_points, (size_t)B * sizeof(int), hipMemcpyHostToDevice, s));
        a.n = c->fn.p;
        if (inputs_on_device) { a.pts = reinterpret_cast<const sind::CloudPoint*>(points); a.stride = stride; }
        else {
            for (int b = 0; b < B; b++) if (hn[b]) HIP_TRY(hipMemcpyAsync(c->fin.p + (size_t)b * c->np, points + (size_t)b * stride, (size_t)hn[b] * sizeof(sind::CloudPoint), hipMemcpyHostToDevice, s));
            a.pts = c->fin.p; a.stride = c->np;
        }
    }
    a.bbox = c->fbbox.p; a.nfin = c->fnfin.p; a.plan = c->fplan.p; a.cellStart = c->fcellStart.p; a.cursor = c->fcursor.p; a.sorted = c->fsorted.p; a.list = c->flist.p; a.listN = c->flistN.p;
    a.dist = c->fdist.p; a.chunkOff = c->fchunkOff.p; a.stats = c->fstats.p; a.nOut = c->fnOut.p; a.out = c->fout.p;
    SIND_TRY(sind::launch_cloud_filter(a, B, nmax, mean_k, stddev_mul, s));
    HIP_TRY(hipMemcpyAsync(c->h_nout.data(), c->fnOut.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
    if (stats) HIP_TRY(hipMemcpyAsync(stats, c->fstats.p, (size_t)B * sizeof(sind::CfStats), hipMemcpyDeviceToHost, s));
    if (distances) for (int b = 0; b < B; b++) if (hn[b]) HIP_TRY(hipMemcpyAsync(distances + (size_t)b * stride, c->fdist.p + (size_t)b * c->np, (size_t)hn[b] * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));                                 // wait 1: the counts
    int rc = SIND_OK;
    for (int b = 0; b < B; b++) {
        n_out[b] = c->h_nout[b];
        if (!out || rc != SIND_OK) continue;
        if (n_out[b] > out_cap) { sind_set_error("sind_cloud_filter_outliers: cloud %d keeps %d points, capacity %d", b, n_out[b], out_cap); rc = SIND_E_CAPACITY; continue; }
        if (n_out[b]) HIP_TRY(hipMemcpyAsync(out + (size_t)b * out_cap, c->fout.p + (size_t)b * c->np, (size_t)n_out[b] * sizeof(sind::CloudPoint), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));                                 // wait 2: the copies sized by them
    return rc;
}

}  // extern "C"
