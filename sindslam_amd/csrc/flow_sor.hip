// The SOR solver of a level: which kernel solves it (sor_plan, the ONE statement of that policy), the launches (sor_iterations), and the two kernels that live here:
// k_sor_color (one launch per colour) and k_sor_fused (one-workgroup levels and 64 x 64 tiles).  The other solver kernels have a file each: flow_stream.hip,
// flow_wave.hip, flow_coarse.hip (k_sor_tile and the chain).
#include "flow_dev.hpp"

namespace sind {

// ---------------------------------------------------------------------------------------------------------
// RedBlackSOR_ParBody: one colour of one SOR iteration (plain version: one thread per pixel of the colour).
// Out-of-image neighbours contribute exactly 0 (zero weight / zero increment in OpenCV's buffer borders).
__global__ void k_sor_color(int w, int h, float omega, int color, const float* __restrict__ A11, const float* __restrict__ A12,
                            const float* __restrict__ A22, const float* __restrict__ B1, const float* __restrict__ B2,
                            const float* __restrict__ Wgt, float* __restrict__ dWu, float* __restrict__ dWv) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    const int x = 2 * k + ((y + color) & 1);
    if (x >= w) return;
    const size_t base = (size_t)b * w * h; const int i = y * w + x;
    const float* Wg = Wgt + base; float* U = dWu + base; float* V = dWv + base;
    const float wp = Wg[i];
    const float wl = x > 0 ? Wg[i - 1] : 0.f, wu = y > 0 ? Wg[i - w] : 0.f;
    const float ul = x > 0 ? U[i - 1] : 0.f, vl = x > 0 ? V[i - 1] : 0.f;
    const float ur = x < w - 1 ? U[i + 1] : 0.f, vr = x < w - 1 ? V[i + 1] : 0.f;
    const float uu = y > 0 ? U[i - w] : 0.f, vu = y > 0 ? V[i - w] : 0.f;
    const float ud = y < h - 1 ? U[i + w] : 0.f, vd = y < h - 1 ? V[i + w] : 0.f;
    const float sigmaU = wl * ul + wp * ur + wu * uu + wp * ud;
    const float sigmaV = wl * vl + wp * vr + wu * vu + wp * vd;
    float du = U[i], dv = V[i];
    const float a12 = A12[base + i];
    du += omega * ((sigmaU + B1[base + i] - dv * a12) / A11[base + i] - du);
    dv += omega * ((sigmaV + B2[base + i] - du * a12) / A22[base + i] - dv);
    U[i] = du; V[i] = dv;
}

// ---------------------------------------------------------------------------------------------------------
// Fused red-black SOR: `iters` full iterations per launch with the linear system held in REGISTERS.
//   * a workgroup owns an extended tile E (EW x EH pixels); every thread owns a 1x8 pixel strip of one row and keeps
//     its 8 x (A11, A12, A22, b1, b2, w, w_up) + w_left in VGPRs for the whole launch (the CU's 512 KB register file is
//     the largest on-chip store; LDS only carries the flow increments);
//   * the increments (du, dv) live in LDS in a checkerboard-split layout (plane[parity][component][row][x/2]) so that the
//     four up / down neighbours of a thread's four same-colour pixels are ONE ds_read_b128 per plane; horizontal
//     neighbours are the thread's own other-colour registers plus one LDS word at the strip edge;
//   * waves are row-parity uniform (first half of the block = even rows, second half = odd rows), so the choice of which
//     four strip pixels carry the active colour is wave-uniform: no divergence;
//   * tiles overlap by a halo of 2*iters pixels: stale values creep inwards one pixel per half-sweep from the tile edge, so
//     the interior (written back) is exact; at image borders E is clipped and the boundary condition is exact.
// Arithmetic per pixel is identical to k_sor_color / OpenCV RedBlackSOR_ParBody, so results stay bit-exact.
#define SOR_PX 8
#define SOR_NT 1024
// Row stride of the LDS planes in float4: strips + a guard on each side, padded to 4 (mod 8).  A wave's ds_read_b128 is served in four 16-lane groups
// that each touch four half rows (16 banks) of four different rows two apart; with a stride of 4 (mod 8) float4 the four pieces fall into the four
// different quarters of the 64 banks (stride 10, the unpadded 64-pixel tile, put two of them on the same quarter: 40 % of the LDS cycles were conflicts).
__host__ __device__ constexpr int sor_row_stride(int EW) { return (EW / 8 + 2) + ((4 - (EW / 8 + 2)) % 8 + 8) % 8; }
__device__ __forceinline__ void ld8(const float* __restrict__ p, float (&d)[SOR_PX]) {
    const F4u a = *reinterpret_cast<const F4u*>(p), c = *reinterpret_cast<const F4u*>(p + 4);
    d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = c.x; d[5] = c.y; d[6] = c.z; d[7] = c.w;
}
// Fused register-resident SOR over one extended tile: the two divisions of a pixel update are Markstein's three-operation sequence on a reciprocal formed
// on the fly (sor_rcp / sor_div: the correctly rounded quotient for |n| >= 2^-100, the IEEE division below; flow_dev.hpp).  MAXT threads per workgroup, WPE waves per SIMD.
// CEW x CNR: extended tile known at compile time (0 = run-time sizes, the one-workgroup levels): every LDS address then is one base register plus an
// immediate offset instead of a dozen address registers held across the loop.
template <int MAXT, int WPE, int CEW, int CNR>
__global__ void __attribute__((amdgpu_flat_work_group_size(64, MAXT), amdgpu_waves_per_eu(WPE, WPE)))
k_sor_fused(int w, int h, int EW, int EH, int IW, int IH, int halo_x, int halo, int ntx, int iters, int xcd_remap, float omega,
            const float* __restrict__ gA11, const float* __restrict__ gA12, const float* __restrict__ gA22, const float* __restrict__ gB1,
            const float* __restrict__ gB2, const float* __restrict__ gW, const float* __restrict__ gUin, const float* __restrict__ gVin,
            float* __restrict__ gUout, float* __restrict__ gVout) {
    extern __shared__ float4 lds4[];             // float4-indexed so that every strip access is one ds_read/write_b128
    float* lds = reinterpret_cast<float*>(lds4);
    const int SW = (CEW ? CEW : EW) / SOR_PX;    // strips per row
    const int RS4 = sor_row_stride(CEW ? CEW : EW);      // LDS row stride in float4 (one guard float4 on each side + bank padding)
    const int half = CEW ? CEW * CNR / (2 * SOR_PX) : (int)(blockDim.x >> 1);
    const int NR = CEW ? CNR : 2 * (half / SW);  // rows covered by the thread block (>= EH; surplus rows stay zero)
    const int PL4 = (NR + 2) * RS4;              // one plane (guard row above and below)
    const int tid = threadIdx.x;
    const int idx = tid < half ? tid : tid - half;
    const int j = idx % SW, ly = 2 * (idx / SW) + (tid < half ? 0 : 1);
    // XCD-aware tile order: workgroups go round-robin to the 8 XCDs (each with its own L2) in linear-id order, so neighbouring ids never
    // share an L2.  Re-map id -> (image, tile) such that XCD q walks the q-th eighth of all tiles in order: tiles that overlap in their
    // halos then run on the same XCD at about the same time and the halo is fetched from HBM once.
    int tile = blockIdx.x, b = blockIdx.y;
    {
        const long long ntile = gridDim.x, lin = blockIdx.x + (long long)blockIdx.y * ntile, per = ntile * gridDim.y / 8;
        if (xcd_remap && lin < per * 8) { const long long logical = (lin & 7) * per + (lin >> 3); b = (int)(logical / ntile); tile = (int)(logical - (long long)b * ntile); }
    }
    const int tx = tile % ntx, ty = tile / ntx;
    const int ex0 = tx * IW - halo_x, ey0 = ty * IH - halo;         // E origin in image coordinates (may be negative)
    const int gy = ey0 + ly, gx0 = ex0 + SOR_PX * j;
    const size_t base = (size_t)b * w * h;
    const int off = (ex0 + ey0) & 1;             // local parity of the globally "red" pixels

    float a11[SOR_PX], a12[SOR_PX], a22[SOR_PX], b1[SOR_PX], b2[SOR_PX], wp[SOR_PX], du[SOR_PX], dv[SOR_PX];
    float wtop[SOR_PX];                          // weights of the image row above the tile, loaded by the tile's first row only
    float wl0 = 0.f;
    unsigned valid = 0;
    const bool row_ok = ly < EH && gy >= 0 && gy < h;
    #pragma unroll
    for (int i = 0; i < SOR_PX; i++) { a11[i] = 1.f; a12[i] = 0.f; a22[i] = 1.f; b1[i] = 0.f; b2[i] = 0.f; wp[i] = 0.f; wtop[i] = 0.f; du[i] = 0.f; dv[i] = 0.f; }
    if (row_ok && gx0 >= 0 && gx0 + SOR_PX <= w) {        // whole strip inside the image: 16-byte loads
        const size_t g = base + (size_t)gy * w + gx0;
        valid = 0xffu;
        ld8(gA11 + g, a11); ld8(gA12 + g, a12); ld8(gA22 + g, a22); ld8(gB1 + g, b1); ld8(gB2 + g, b2); ld8(gW + g, wp); ld8(gUin + g, du); ld8(gVin + g, dv);
        if (ly == 0 && gy > 0) ld8(gW + g - w, wtop);
    } else if (row_ok) {
        #pragma unroll
        for (int i = 0; i < SOR_PX; i++) {
            const int gx = gx0 + i;
            if (gx >= 0 && gx < w) {
                const size_t g = base + (size_t)gy * w + gx;
                valid |= 1u << i;
                a11[i] = gA11[g]; a12[i] = gA12[g]; a22[i] = gA22[g]; b1[i] = gB1[g]; b2[i] = gB2[g]; wp[i] = gW[g];
                if (ly == 0 && gy > 0) wtop[i] = gW[g - w];
                du[i] = gUin[g]; dv[i] = gVin[g];
            }
        }
    }
    // zero the guard ring of the six planes (top and bottom row, the cells left and right of the strips; every other cell is written below by the
    // thread that owns it) while the loads above are in flight
    {
        const int GC = RS4 - SW, G = 2 * RS4 + NR * GC;          // guard cells per row / per plane
        for (int i = tid; i < 6 * G; i += blockDim.x) {
            const int pl = i / G, c = i - pl * G;
            int cell;
            if (c < 2 * RS4) cell = c < RS4 ? c : (NR + 1) * RS4 + (c - RS4);
            else { const int r = (c - 2 * RS4) / GC, g = (c - 2 * RS4) - r * GC; cell = (r + 1) * RS4 + (g == 0 ? 0 : SW + g); }
            lds4[pl * PL4 + cell] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    __syncthreads();
    // LDS addressing (float4 units): plane(parity q, component c) at (q*2 + c)*PL4; strip j of row ly at (ly+1)*RS4 + 1 + j
    const int ro4 = (ly + 1) * RS4 + 1 + j;
    const int s0 = ly & 1;                       // strip pixels i with ((i + ly) & 1) == q have local parity q
    {   // initial state of both parities: strip pixels s0, s0+2, ... are local-even, the others local-odd
        const float4 au = make_float4(du[0], du[2], du[4], du[6]), bu = make_float4(du[1], du[3], du[5], du[7]);
        const float4 av = make_float4(dv[0], dv[2], dv[4], dv[6]), bv = make_float4(dv[1], dv[3], dv[5], dv[7]);
        const int pe = s0 == 0 ? 0 : 2, po = s0 == 0 ? 2 : 0;      // plane pair receiving the i-even / i-odd pixels
        lds4[(pe + 0) * PL4 + ro4] = au; lds4[(pe + 1) * PL4 + ro4] = av;
        lds4[(po + 0) * PL4 + ro4] = bu; lds4[(po + 1) * PL4 + ro4] = bv;
        // smoothness weights, same checkerboard split (plane 4 + parity): a pixel's upper weight is read back from the row above, so the
        // w_up plane is neither loaded from memory (one ninth of the tile's load requests) nor held in registers
        lds4[(4 + (pe >> 1)) * PL4 + ro4] = make_float4(wp[0], wp[2], wp[4], wp[6]);
        lds4[(4 + (po >> 1)) * PL4 + ro4] = make_float4(wp[1], wp[3], wp[5], wp[7]);
        if (ly == 0) {                           // guard row = image row above the tile: pixel parities are those of local row -1
            lds4[(4 + (po >> 1)) * PL4 + ro4 - RS4] = make_float4(wtop[0], wtop[2], wtop[4], wtop[6]);
            lds4[(4 + (pe >> 1)) * PL4 + ro4 - RS4] = make_float4(wtop[1], wtop[3], wtop[5], wtop[7]);
        }
    }
    __syncthreads();
    // weight of the pixel left of the strip = last pixel of the neighbouring strip (LDS); at the tile's left edge it reads the zero
    // guard, which only touches the outermost halo ring (never part of the written interior) or lies outside the image (weight 0)
    wl0 = lds[4 * ((4 + (s0 ^ 1)) * PL4 + ro4) - 1];

    // one half-sweep over the strip pixels START, START+2, START+4, START+6 (compile-time START keeps register indices static);
    // Q = local parity being updated.  Invalid pixels (outside the image / surplus rows) keep du = dv = 0.
    #define SOR_HALF(START, Q)                                                                                                    \
        {                                                                                                                         \
            const int oq = (Q) ^ 1;                                                                                               \
            const float4 t0 = lds4[(oq * 2 + 0) * PL4 + ro4 - RS4], t1 = lds4[(oq * 2 + 1) * PL4 + ro4 - RS4];                    \
            const float4 t2 = lds4[(oq * 2 + 0) * PL4 + ro4 + RS4], t3 = lds4[(oq * 2 + 1) * PL4 + ro4 + RS4];                    \
            const float uu[4] = {t0.x, t0.y, t0.z, t0.w}, vu[4] = {t1.x, t1.y, t1.z, t1.w};                                       \
            const float ud[4] = {t2.x, t2.y, t2.z, t2.w}, vd[4] = {t3.x, t3.y, t3.z, t3.w};                                       \
            const float4 tw = lds4[(4 + oq) * PL4 + ro4 - RS4]; const float wu[4] = {tw.x, tw.y, tw.z, tw.w};                     \
            /* strip-edge horizontal neighbour: left of pixel 0 (START == 0) or right of pixel 7 (START == 1) */                   \
            const float eu = lds[4 * ((oq * 2 + 0) * PL4 + ro4) + ((START) == 0 ? -1 : 4)];                                       \
            const float ev = lds[4 * ((oq * 2 + 1) * PL4 + ro4) + ((START) == 0 ? -1 : 4)];                                       \
            _Pragma("unroll")                                                                                                     \
            for (int k = 0; k < 4; k++) {                                                                                         \
                const int i = (START) + 2 * k;                                                                                    \
                const float wl = i == 0 ? wl0 : wp[i == 0 ? 0 : i - 1];                                                           \
                const float ul = i == 0 ? eu : du[i == 0 ? 0 : i - 1], vl = i == 0 ? ev : dv[i == 0 ? 0 : i - 1];                \
                const float ur = i == 7 ? eu : du[i == 7 ? 7 : i + 1], vr = i == 7 ? ev : dv[i == 7 ? 7 : i + 1];                \
                const float sigmaU = wl * ul + wp[i] * ur + wu[k] * uu[k] + wp[i] * ud[k];                                        \
                const float sigmaV = wl * vl + wp[i] * vr + wu[k] * vu[k] + wp[i] * vd[k];                                        \
                float nu = du[i], nv = dv[i];                                                                                     \
                sor_update(nu, nv, sigmaU + b1[i], sigmaV + b2[i], a12[i], a11[i], sor_rcp(a11[i]), a22[i], sor_rcp(a22[i]), omega);     \
                const bool ok = (valid >> i) & 1u;                                                                                \
                du[i] = ok ? nu : 0.f; dv[i] = ok ? nv : 0.f;                                                                     \
            }                                                                                                                     \
            lds4[((Q) * 2 + 0) * PL4 + ro4] = make_float4(du[START], du[(START) + 2], du[(START) + 4], du[(START) + 6]);         \
            lds4[((Q) * 2 + 1) * PL4 + ro4] = make_float4(dv[START], dv[(START) + 2], dv[(START) + 4], dv[(START) + 6]);         \
        }

    // globally red pixels have local parity `off`; in this thread's row they are the strip pixels i == c (mod 2), c wave-uniform
    if ((off ^ s0) == 0) {
        for (int it = 0; it < iters; it++) { SOR_HALF(0, off) __syncthreads(); SOR_HALF(1, off ^ 1) __syncthreads(); }
    } else {
        for (int it = 0; it < iters; it++) { SOR_HALF(1, off) __syncthreads(); SOR_HALF(0, off ^ 1) __syncthreads(); }
    }
    #undef SOR_HALF
    if (row_ok) {
        const int ix0 = tx * IW, iy0 = ty * IH;
        if (gy >= iy0 && gy < iy0 + IH) {
            // 16-byte stores for the half strips that lie inside the written interior (the interior starts at a multiple of 44 = 4 x 11 pixels, so its
            // quads are whole): the per-pixel stores of a whole strip cost the L2 ~17 masked 64-byte write requests per wave instruction, and the
            // write requests outnumbered the read requests of the tile loads (TCP_TCC_WRITE_REQ 1.17e10 vs READ 1.02e10 over the same launches)
            #pragma unroll
            for (int q = 0; q < SOR_PX; q += 4) {
                const int gxa = gx0 + q; const size_t g = base + (size_t)gy * w + gxa;
                if (((valid >> q) & 0xfu) == 0xfu && gxa >= ix0 && gxa + 4 <= ix0 + IW) {
                    *reinterpret_cast<F4u*>(gUout + g) = F4u{du[q], du[q + 1], du[q + 2], du[q + 3]};
                    *reinterpret_cast<F4u*>(gVout + g) = F4u{dv[q], dv[q + 1], dv[q + 2], dv[q + 3]};
                } else {
                    #pragma unroll
                    for (int i = q; i < q + 4; i++) {
                        const int gx = gx0 + i;
                        if (((valid >> i) & 1u) && gx >= ix0 && gx < ix0 + IW) { gUout[g + (i - q)] = du[i]; gVout[g + (i - q)] = dv[i]; }
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// k_sor_fused's geometry: threads of an EW x EH extended tile (whole waves per row parity), LDS bytes of a block of nt threads, and the attribute both launchers need
static int sor_fused_threads(int EW, int EH) { const int halfn = (EW / SOR_PX) * ((EH + 1) / 2); return 2 * ((halfn + 63) / 64 * 64); }
static size_t sor_fused_lds(int EW, int nt) { const int NR = 2 * ((nt / 2) / (EW / SOR_PX)); return (size_t)6 * (NR + 2) * sor_row_stride(EW) * sizeof(float4); }
static int sor_fused_attr() {
    // the flow slices call this concurrently from their own threads: set the (idempotent) attribute once per device
    static SindPerDeviceInit attr_init;
    HIP_TRY(attr_init.run([] {
        hipError_t attr_rc = hipSuccess;
        const void* fs[] = {(const void*)k_sor_fused<1024, 4, 0, 0>, (const void*)k_sor_fused<512, 2, 0, 0>, (const void*)k_sor_fused<512, 4, 64, 64>};
        for (const void* f : fs) if (attr_rc == hipSuccess) attr_rc = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
        return attr_rc;
    }));
    return SIND_OK;
}
// one iteration, one launch per colour, in place
static int launch_sor_color(hipStream_t s, FlowPlanes& P, int w, int h, int B, float omega) {
    const dim3 gs(divup(divup(w, 2), 64), h, B), bs(64);
    hipLaunchKernelGGL(k_sor_color, gs, bs, 0, s, w, h, omega, 0, P.A11, P.A12, P.A22, P.b1, P.b2, P.wgt, P.dWu, P.dWv);
    hipLaunchKernelGGL(k_sor_color, gs, bs, 0, s, w, h, omega, 1, P.A11, P.A12, P.A22, P.b1, P.b2, P.wgt, P.dWu, P.dWv);
    return SIND_OK;
}
// whole image in one workgroup: every iteration in one launch, in place
static int launch_sor_fused_level(hipStream_t s, FlowPlanes& P, int w, int h, int B, int iters, float omega) {
    const int EW = (w + SOR_PX - 1) / SOR_PX * SOR_PX, EH = h, nt = sor_fused_threads(EW, EH);
    SIND_TRY(sor_fused_attr());
    // <= 512 threads: two waves per SIMD, i.e. up to 256 registers -- room for the run-time tile sizes AND the reciprocal division without spills
    // (all 25 iterations run in this launch, so here the loop is the cost); larger blocks run four waves per SIMD
    auto kern1 = nt <= 512 ? k_sor_fused<512, 2, 0, 0> : k_sor_fused<1024, 4, 0, 0>;
    hipLaunchKernelGGL(kern1, dim3(1, B), dim3(nt), sor_fused_lds(EW, nt), s, w, h, EW, EH, EW, EH, 0, 0, 1, iters, 0, omega, P.A11, P.A12, P.A22, P.b1, P.b2, P.wgt,
                       P.dWu, P.dWv, P.dWu, P.dWv);
    return SIND_OK;
}
// tiled levels: EW x EH tiles of EW * EH / 8 threads, four waves per SIMD, k iterations on a halo of 2 k pixels, ping-pong between the two increment buffers
// (a tile reads its halo from neighbours that another workgroup of the same launch rewrites)
static int launch_sor_fused_tiles(hipStream_t s, FlowPlanes& P, int w, int h, int B, int k, float omega, const SolverCfg& C) {
    const int EW = C.tile_w, EH = C.tile_h, nt = sor_fused_threads(EW, EH);
    SIND_TRY(sor_fused_attr());
    const bool t64 = EW == 64 && EH == 64 && nt == 512;               // the default tile has an instance with compile-time sizes
    auto kern = t64 ? k_sor_fused<512, 4, 64, 64> : k_sor_fused<1024, 4, 0, 0>;
    const int halo = 2 * k, halo_x = halo, IW = EW - 2 * halo_x, IH = EH - 2 * halo;
    const int ntx = divup(w, IW), nty = divup(h, IH);
    hipLaunchKernelGGL(kern, dim3(ntx * nty, B), dim3(nt), sor_fused_lds(EW, nt), s, w, h, EW, EH, IW, IH, halo_x, halo, ntx, k, 1, omega, P.A11, P.A12, P.A22, P.b1, P.b2,
                       P.wgt, P.dWu, P.dWv, P.dWu2, P.dWv2);
    std::swap(P.dWu, P.dWu2); std::swap(P.dWv, P.dWv2);
    return SIND_OK;
}

// ---------------------------------------------------------------------------------------------------------
// The policy.  (The solver settings -- variant, iterations per launch, tile, large-level threshold -- are a SolverCfg per flow handle: flow.hpp.)
// Few images: the launch is latency-bound (a tile per compute unit, most of the chip idle).  Then 1024-thread tiles (k_sor_tile) run MORE iterations per launch on deeper
// halos: the fewest launches whose tiles all still find a compute unit of their own (a launch costs ~6 us before its first iteration; an iteration ~0.8 us).
// Returns the iterations of each launch, or nothing if the level at this batch size is throughput-bound.
static std::vector<int> sor_latency_plan(int w, int h, int B, int total) {
    const int slots = 256;                                   // compute units: one 1024-thread workgroup each
    for (int n = 1; n <= total; n++) {
        const int base = total / n, rem = total % n, kmax = base + (rem ? 1 : 0);
        if (kmax > 13) continue;                             // 64 - 4 k >= 12 kept pixels per tile edge
        if ((long long)sor_tile_count(w, h, kmax) * B > slots) { if (kmax <= 5) break; continue; }
        std::vector<int> plan((size_t)n, base);
        for (int i = 0; i < rem; i++) plan[(size_t)i]++;
        return plan;
    }
    return {};
}
bool chain_takes_level(int w, int h, float epsilon, const SolverCfg& C) { return C.coarse_chain && epsilon >= 1e-12f && coarse_level_P(w, h) != 0; }
int sor_plan(int w, int h, int B, int total, float epsilon, const SolverCfg& C, SorPlan* plan) {
    auto is = [&](SorKernel k, std::vector<int> iters) { plan->kernel = k; plan->iters = std::move(iters); return SIND_OK; };
    total = std::max(total, 0);
    if (C.mode == 0) return is(SOR_COLOR, std::vector<int>((size_t)total, 1));
    if (chain_takes_level(w, h, epsilon, C)) return is(SOR_COARSE_CHAIN, {total});       // one workgroup's work: the whole level in one launch (flow_coarse.hip)
    const int EWw = (w + SOR_PX - 1) / SOR_PX * SOR_PX, nt1 = sor_fused_threads(EWw, h);
    if (C.latency_tiles && C.mode == 4) {       // (mode 5 asks for the streaming kernel wherever it fits)
        std::vector<int> lat = sor_latency_plan(w, h, B, total);
        if (!lat.empty() && !(lat.size() > 1 && nt1 <= 512)) return is(SOR_LATENCY_TILES, std::move(lat));      // (a level of <= 4096 pixels that is not in the chain: one launch of the one-workgroup kernel is as good)
    }
    if (nt1 <= SOR_NT) {
        const size_t shm = sor_fused_lds(EWw, nt1);
        if (shm > 150 * 1024) { sind_set_error("sor_iterations: a %d x %d level needs %zu bytes of LDS", w, h, shm); return SIND_E_ARG; }
        return is(SOR_ONE_WORKGROUP, {total});
    }
    const bool large = C.mode == 4 && B >= C.stream_min_b;      // large levels, many images
    // one-wave row pipelines (flow_wave.hip) -- no workgroup barrier anywhere
    if (total % 5 == 0 && (C.mode == 6 || (large && C.wave))) return is(SOR_WAVE, std::vector<int>((size_t)(total / 5), 5));
    // ... or the streaming kernel (one workgroup per image and column strip; no halo, loads and stores overlapped with the iterations)
    if (sor_stream_fits(h, total) && (C.mode == 5 || large)) return is(SOR_STREAM, std::vector<int>((size_t)(total / 5), 5));
    // the tiled kernel: C.fuse iterations per launch (the last launch of a level takes the rest)
    const int EW = C.tile_w, EH = C.tile_h, nt = sor_fused_threads(EW, EH);
    if (nt > SOR_NT || 2 * 2 * C.fuse >= std::min(EW, EH)) { sind_set_error("sor_iterations: tile %d x %d / %d fused iterations not supported", EW, EH, C.fuse); return SIND_E_ARG; }
    const size_t shm = sor_fused_lds(EW, nt);
    if (shm > 150 * 1024) { sind_set_error("sor_iterations: %d x %d tiles need %zu bytes of LDS", EW, EH, shm); return SIND_E_ARG; }
    std::vector<int> tiles;
    for (int done = 0; done < total; done += tiles.back()) tiles.push_back(std::min(C.fuse, total - done));
    return is(SOR_FUSED_TILES, std::move(tiles));
}

// The plan's launches on the level's system; every launcher owns its kernel's geometry.  *nlaunch counts kernels.
int sor_iterations(hipStream_t s, FlowPlanes& P, int w, int h, int B, float omega, const SorPlan& plan, const SolverCfg& C, long long* nlaunch) {
    for (int k : plan.iters) {
        switch (plan.kernel) {
            case SOR_COLOR:         SIND_TRY(launch_sor_color(s, P, w, h, B, omega)); *nlaunch += 1; break;
            case SOR_LATENCY_TILES: SIND_TRY(launch_sor_tile(s, P, w, h, B, k, omega)); break;
            case SOR_ONE_WORKGROUP: SIND_TRY(launch_sor_fused_level(s, P, w, h, B, k, omega)); break;
            case SOR_WAVE:          SIND_TRY(launch_sor_wave(s, P, w, h, B, omega, C.wave_items, C.wave_bands, C.wave_prefetch, C.wave_group)); break;
            case SOR_STREAM:        SIND_TRY(launch_sor_stream(s, P, w, h, B, omega, C.stream_wg_cap)); break;
            case SOR_FUSED_TILES:   SIND_TRY(launch_sor_fused_tiles(s, P, w, h, B, k, omega, C)); break;
            default: sind_set_error("sor_iterations: the coarse chain solves its levels itself"); return SIND_E_ARG;
        }
        *nlaunch += 1;
    }
    return SIND_OK;
}

}  // namespace sind
