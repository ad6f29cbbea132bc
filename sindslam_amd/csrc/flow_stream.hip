// k_sor_stream: the large levels as one 512-thread workgroup per (column strip, image) -- the cross-check of k_sor_wave (flow_wave.hip), behind
// sind_flow_set_wave_solver(f, 0, ...) and mode 5.
#include "flow_dev.hpp"

namespace sind {

// ---------------------------------------------------------------------------------------------------------
// Third generation for the large levels: the solver STREAMS down the image instead of tiling it.
// The tiled kernel (k_sor_fused, flow_sor.hip) pays for its halo twice: a 64 x 64 tile with a 10-pixel halo computes (64 / 44)^2 = 2.1 x the pixel updates it keeps, and a
// workgroup can neither load the next tile's coefficients nor store its result while it iterates (loads + write-back are 58 % of a tiled launch).
// Here ONE workgroup owns one column strip of an image (up to 152 columns: 128 kept + 12 halo columns on each cut side) and walks it top to bottom as a
// software pipeline in time:
//   * half-sweep s (s = 0 .. 2 * iters - 1, red first) of image row y runs at step t = y + 2 s.  Row y then has rows y - 1 and y + 1 exactly after
//     half-sweep s - 1 and before s + 1 -- what the sequential red-black order defines -- and the rows updated in one step (all of t's parity) never
//     read each other: every pixel update is the same arithmetic on the same operands as in k_sor_color, so the result is bit-identical, with NO
//     redundant update and every coefficient read from memory exactly once per launch;
//   * a thread owns a 1 x 4 strip of TWO consecutive rows (2 p, 2 p + 1) for the SS_NQ steps they spend in the pipeline (every step: a half-sweep of its odd
//     row, then one of its even row), keeps their system AND their du / dv in registers, then takes the pair SS_NQ pairs further down;
//   * du, dv and the smoothness weight also live in LDS rings of SS_RING rows, split by column parity (the two pixels a strip updates in a half-sweep and
//     their vertical neighbours are one 8-byte access per plane): a thread reads from them only what OTHER threads own -- the row above its even row, the
//     row below its odd row and the strip-edge neighbours; threads are grouped by the parity of their pair slot (whole waves per group) so that the active
//     colour is a scalar per wave;
//   * the rows ahead of the pipeline are fetched by two LOADER waves (one per row of a pair): every step a loader parks the 16-byte pieces it requested two
//     steps earlier in LDS (coefficients and the reciprocals of A11 / A22, which it forms: staging ring, read once by the row's next owner; du / dv / w:
//     the rings) and requests the pieces of the pair three steps ahead.  The step barrier waits for LDS only (s_waitcnt lgkmcnt(0); s_barrier), so those
//     loads stay in flight across steps.  (One loader wave for both rows was the step time: DESIGN 3.1-9, profiles/r03/v2_step_probes.txt);
//   * a finished row goes from LDS to the output planes (ping-pong with the input: neighbouring column strips read each other's halo columns).
#define SS_NQ 10           /* pair slots = rows in flight / 2 = half-sweeps per launch (5 iterations) */
#define SS_RING 28         /* rows of du / dv / w resident in LDS: the rows of pair p are parked during step p - 1 and read until step p + SS_NQ */
#define SS_STG 4           /* rows of the coefficient staging ring */
#define SS_MAXSW 38        /* widest column strip in 4-pixel strips: 6 compute waves + 2 loader waves = 512 threads, two workgroups per CU */
#define SS_NST 7           /* staging planes: A11, A12, A22, b1, b2 and the reciprocals of A11 and A22 (formed by the loader wave) */
typedef float ss_f4 __attribute__((ext_vector_type(4)));
typedef float ss_f2 __attribute__((ext_vector_type(2)));
typedef float ss_f2a __attribute__((ext_vector_type(2), aligned(4)));      // two neighbouring floats at any 4-byte address (ds_read2_b32)
__device__ __forceinline__ void ss_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
struct SsRow { float a11[4], a12[4], a22[4], b1[4], b2[4], wp[4], r11[4], r22[4], du[4], dv[4]; float wl0; };      // du / dv: the owner's copy (the rings hold the same values for the neighbours and the write-back); r = RN(1 / a), formed once per row by the loader wave (0 for a pixel outside the image: its update returns exactly 0)
// MAXSW: widest column strip (in 4-pixel strips) the instance is laid out for.  The LDS layout is fixed at compile time (every plane at a constant offset:
// an access is one base register per ring row plus an immediate); 38 strips = 152 columns need 69 KB and 512 threads (6 compute waves + 2 loaders):
// two workgroups per CU.  Wider levels are cut into column strips (grid x), each with its own pipeline.
// One (column strip, image) of a launch: the whole row pipeline of that strip, top to bottom.
template <int MAXSW>
__device__ __forceinline__ void ss_item(float* lds, const int strip, const int image, int w, int h, int SW, int HT, int IW, float omega, const float* __restrict__ gA11, const float* __restrict__ gA12,
                                                     const float* __restrict__ gA22, const float* __restrict__ gB1, const float* __restrict__ gB2,
                                                     const float* __restrict__ gW, const float* __restrict__ gU, const float* __restrict__ gV, float* __restrict__ gUo, float* __restrict__ gVo) {
    constexpr int HS = 2 * MAXSW + 4, EWS = 4 * MAXSW;            // floats per row: split plane (two guard floats on each side), staging
    constexpr int PL = SS_RING * HS;                              // one parity plane of a ring
    constexpr int O_DU = 2, O_DV = 2 * PL + 2, O_W = 4 * PL + 2, O_ST = 6 * PL, STP = SS_STG * EWS;      // float offsets (rings: + parity * PL + slot * HS + x / 2)
    constexpr int total = 6 * PL + SS_NST * STP;
    int tid_ = threadIdx.x; asm volatile("" : "+v"(tid_));     // (opaque per item: nothing derived from it is hoisted out of the kernel's item loop and kept in registers across items)
    const int tid = tid_;
    const size_t base = (size_t)image * w * h;
    // column strip of this workgroup: it keeps the columns [ix0, ix1) and works on [ex0, ex0 + 4 SW), 12 columns more on every side that is not an image
    // border (a cut edge reads zeros from outside; what that falsifies creeps inwards one column per half-sweep, 10 columns in a launch; 12 keeps ex0 a multiple of 4)
    const int ix0 = strip * IW, ix1 = min(ix0 + IW, w), ex0 = max(ix0 - 12, 0);
    for (int i = tid; i < total; i += blockDim.x) lds[i] = 0.f;   // guards, the row above the image, and everything not yet loaded read as zero
    // roles: threads [0, 10 SW) compute -- slot group g (parity of the pair index: first 5 SW threads even slots, next 5 SW odd), slot within the group, strip;
    // the LAST TWO waves of the block are the loaders, one for the even and one for the odd row of every pair (their own registers hold two rows of 16-byte
    // pieces in flight each; the compute waves hold none).  One loader wave for both rows ran ~3500 cycles a step against ~1900 of a compute wave and was
    // the step time (in-kernel clock probes, profiles/r03/v2_step_probes.txt)
    const int CT = (int)blockDim.x - 128;                         // compute threads (padded to whole waves)
    const int lw = (tid - CT) >> 6;                               // loader index (0, 1) if this wave loads
    const bool is_loader = tid >= CT;
    const int ct = tid;
    const int g = ct >= HT ? 1 : 0, idx = g ? ct - HT : ct, qs = idx / SW, j = idx - qs * SW;
    int p = (!is_loader && qs < SS_NQ / 2) ? 2 * qs + g : (1 << 28);      // current row pair; padding lanes and the loader never get one
    const int k2 = 2 * j, x0 = 4 * j;
    // loader: lane l takes the items l, l + 64, ... of a row's 8 SW pieces (plane 0..4 coefficients, 5 weight, 6 du, 7 dv; 4-pixel chunk)
    const int llane = tid & 63, lrow = lw;
    constexpr int SS_NC = (8 * MAXSW + 63) / 64;                  // pieces per loader lane and row
    ss_f4 pf[2][SS_NC];                                           // [step parity][piece]: this loader's row of two row pairs in flight
    #pragma unroll
    for (int a = 0; a < 2; a++) {
        #pragma unroll
        for (int c = 0; c < SS_NC; c++) pf[a][c] = ss_f4{0.f, 0.f, 0.f, 0.f};
    }
    SsRow A, B;
    #pragma unroll
    for (int i = 0; i < 4; i++) { A.a11[i] = A.a22[i] = B.a11[i] = B.a22[i] = 1.f; A.a12[i] = A.b1[i] = A.b2[i] = A.wp[i] = A.r11[i] = A.r22[i] = 0.f; B.a12[i] = B.b1[i] = B.b2[i] = B.wp[i] = B.r11[i] = B.r22[i] = 0.f; }
    A.wl0 = B.wl0 = 0.f;
    #pragma unroll
    for (int i = 0; i < 4; i++) A.du[i] = A.dv[i] = B.du[i] = B.dv[i] = 0.f;
    unsigned smask = 0u;                                         // strip pixels inside the columns this workgroup keeps
    #pragma unroll
    for (int i = 0; i < 4; i++) if (ex0 + x0 + i >= ix0 && ex0 + x0 + i < ix1) smask |= 1u << i;
    __syncthreads();

    // row ROWY (ring slot SLOT) leaves LDS for registers (its owner, at the row's first step)
    #define SS_LOAD(R, ROWY, RB)                                                                                                   \
        {                                                                                                                          \
            const float* st_ = lds + O_ST + ((ROWY) & (SS_STG - 1)) * EWS + k2; const float* rb_ = (RB);                          \
            /* the staging rows are split by column parity like the rings: (pixel 0, pixel 2) and (pixel 1, pixel 3) arrive as the register pairs the    \
               packed FP32 operations of a half-sweep take (a float4 per plane left the pairs to be rebuilt by moves in every half-sweep) */            \
            const float2 e0 = *reinterpret_cast<const float2*>(st_), o0 = *reinterpret_cast<const float2*>(st_ + EWS / 2);                             \
            const float2 e1 = *reinterpret_cast<const float2*>(st_ + STP), o1 = *reinterpret_cast<const float2*>(st_ + STP + EWS / 2);                 \
            const float2 e2 = *reinterpret_cast<const float2*>(st_ + 2 * STP), o2 = *reinterpret_cast<const float2*>(st_ + 2 * STP + EWS / 2);         \
            const float2 e3 = *reinterpret_cast<const float2*>(st_ + 3 * STP), o3 = *reinterpret_cast<const float2*>(st_ + 3 * STP + EWS / 2);         \
            const float2 e4 = *reinterpret_cast<const float2*>(st_ + 4 * STP), o4 = *reinterpret_cast<const float2*>(st_ + 4 * STP + EWS / 2);         \
            const float2 e5 = *reinterpret_cast<const float2*>(st_ + 5 * STP), o5 = *reinterpret_cast<const float2*>(st_ + 5 * STP + EWS / 2);         \
            const float2 e6 = *reinterpret_cast<const float2*>(st_ + 6 * STP), o6 = *reinterpret_cast<const float2*>(st_ + 6 * STP + EWS / 2);         \
            const float2 we = *reinterpret_cast<const float2*>(rb_ + O_W), wo = *reinterpret_cast<const float2*>(rb_ + O_W + PL); \
            R.wl0 = rb_[O_W + PL - 1];                                                                                             \
            const float2 ue_ = *reinterpret_cast<const float2*>(rb_ + O_DU), uo_ = *reinterpret_cast<const float2*>(rb_ + O_DU + PL); \
            const float2 ve_ = *reinterpret_cast<const float2*>(rb_ + O_DV), vo_ = *reinterpret_cast<const float2*>(rb_ + O_DV + PL); \
            R.du[0] = ue_.x; R.du[2] = ue_.y; R.du[1] = uo_.x; R.du[3] = uo_.y; R.dv[0] = ve_.x; R.dv[2] = ve_.y; R.dv[1] = vo_.x; R.dv[3] = vo_.y; \
            R.a11[0] = e0.x; R.a11[2] = e0.y; R.a11[1] = o0.x; R.a11[3] = o0.y; R.a12[0] = e1.x; R.a12[2] = e1.y; R.a12[1] = o1.x; R.a12[3] = o1.y; \
            R.a22[0] = e2.x; R.a22[2] = e2.y; R.a22[1] = o2.x; R.a22[3] = o2.y; R.b1[0] = e3.x; R.b1[2] = e3.y; R.b1[1] = o3.x; R.b1[3] = o3.y;     \
            R.b2[0] = e4.x; R.b2[2] = e4.y; R.b2[1] = o4.x; R.b2[3] = o4.y;                                                        \
            R.wp[0] = we.x; R.wp[2] = we.y; R.wp[1] = wo.x; R.wp[3] = wo.y;                                                        \
            R.r11[0] = e5.x; R.r11[2] = e5.y; R.r11[1] = o5.x; R.r11[3] = o5.y; R.r22[0] = e6.x; R.r22[2] = e6.y; R.r22[1] = o6.x; R.r22[3] = o6.y; \
        }
    // one half-sweep of a row: the two strip pixels of column parity START (the strip starts at an even column).  The thread holds the values of its two rows
    // in registers (the rings carry the same values for the neighbours): the odd row reads its upper neighbour and that row's weights from the even row's
    // registers, the even row its lower neighbour from the odd row's; LDS gives only the row of the OTHER thread (above the even row, below the odd one) and
    // the strip-edge neighbour.  UU / VU / WU, UD / VD: the vertical neighbours' values at the two updated columns.
    #define SS_UPDATE(R, RB, START, UU0, UU1, VU0, VU1, WU0, WU1, UD0, UD1, VD0, VD1)                                              \
        {                                                                                                                          \
            float* rb_ = (RB) + (START) * PL;                                                                                      \
            /* strip-edge horizontal neighbour: left of pixel 0 (an odd column) or right of pixel 3 (the next strip's first, even column) */ \
            /* ... read TOGETHER with the own pixel beside it (pixel 1 resp. pixel 2: the ring holds the thread's own values too, written a step ago), as the register pair the   \
               packed operations take: (edge, 1) resp. (2, edge) used to be put together by two moves per plane and half-sweep */                                              \
            const ss_f2a eup = *reinterpret_cast<const ss_f2a*>((START) == 0 ? rb_ + O_DU + PL - 1 : rb_ + O_DU - PL + 1);           \
            const ss_f2a evp = *reinterpret_cast<const ss_f2a*>((START) == 0 ? rb_ + O_DV + PL - 1 : rb_ + O_DV - PL + 1);           \
            const float uua[2] = {UU0, UU1}, uda[2] = {UD0, UD1}, vua[2] = {VU0, VU1}, vda[2] = {VD0, VD1}, wua[2] = {WU0, WU1};     \
            /* START 0: pixels 0, 2 between (edge, 1) and (1, 3); START 1: pixels 1, 3 between (0, 2) and (2, edge) */             \
            const float ula[2] = {(START) == 0 ? eup.x : R.du[0], (START) == 0 ? eup.y : R.du[2]}, ura[2] = {(START) == 0 ? R.du[1] : eup.x, (START) == 0 ? R.du[3] : eup.y}; \
            const float vla[2] = {(START) == 0 ? evp.x : R.dv[0], (START) == 0 ? evp.y : R.dv[2]}, vra[2] = {(START) == 0 ? R.dv[1] : evp.x, (START) == 0 ? R.dv[3] : evp.y}; \
            _Pragma("unroll")                                                                                                      \
            for (int k = 0; k < 2; k++) {                                                                                          \
                const int i = (START) + 2 * k;                                                                                     \
                const float wl = i == 0 ? R.wl0 : R.wp[i == 0 ? 0 : i - 1];                                                        \
                const float sigmaU = wl * ula[k] + R.wp[i] * ura[k] + wua[k] * uua[k] + R.wp[i] * uda[k];                          \
                const float sigmaV = wl * vla[k] + R.wp[i] * vra[k] + wua[k] * vua[k] + R.wp[i] * vda[k];                          \
                float nu = R.du[i], nv = R.dv[i];                                                                                  \
                sor_update(nu, nv, sigmaU + R.b1[i], sigmaV + R.b2[i], R.a12[i], R.a11[i], R.r11[i], R.a22[i], R.r22[i], omega);          \
                R.du[i] = nu; R.dv[i] = nv;                                                                                        \
            }                                                                                                                      \
            /* (one 8-byte vector store each: as HIP float2 structs the stores were split into scalars, sunk below the two colours' code and came out as four ds_write_b32 with four address adds) */ \
            *reinterpret_cast<ss_f2*>(rb_ + O_DU) = ss_f2{R.du[START], R.du[(START) + 2]}; *reinterpret_cast<ss_f2*>(rb_ + O_DV) = ss_f2{R.dv[START], R.dv[(START) + 2]}; \
        }
    #define SS_HALF_A(START)                                                                                                       \
        {                                                                                                                          \
            const float* ru_ = pU + (START) * PL;                                                                                  \
            const float2 uu = *reinterpret_cast<const float2*>(ru_ + O_DU), vu = *reinterpret_cast<const float2*>(ru_ + O_DV), wu = *reinterpret_cast<const float2*>(ru_ + O_W); \
            SS_UPDATE(A, pA, START, uu.x, uu.y, vu.x, vu.y, wu.x, wu.y, B.du[START], B.du[(START) + 2], B.dv[START], B.dv[(START) + 2]) \
        }
    #define SS_HALF_B(START)                                                                                                       \
        {                                                                                                                          \
            const float* rd_ = pD + (START) * PL;                                                                                  \
            const float2 ud = *reinterpret_cast<const float2*>(rd_ + O_DU), vd = *reinterpret_cast<const float2*>(rd_ + O_DV);     \
            SS_UPDATE(B, pB, START, A.du[START], A.du[(START) + 2], A.dv[START], A.dv[(START) + 2], A.wp[START], A.wp[(START) + 2], ud.x, ud.y, vd.x, vd.y) \
        }
    // a finished row: LDS (both column parities) -> global memory
    #define SS_STORE(ROWY, RB)                                                                                                     \
        {                                                                                                                          \
            const float* rb_ = (RB);                                                                                               \
            const float2 ue = *reinterpret_cast<const float2*>(rb_ + O_DU), uo = *reinterpret_cast<const float2*>(rb_ + O_DU + PL); \
            const float2 ve = *reinterpret_cast<const float2*>(rb_ + O_DV), vo = *reinterpret_cast<const float2*>(rb_ + O_DV + PL); \
            const float du_[4] = {ue.x, uo.x, ue.y, uo.y}, dv_[4] = {ve.x, vo.x, ve.y, vo.y};                                       \
            const size_t go = base + (size_t)(ROWY) * w + ex0 + x0;                                                                \
            if (smask == 0xfu) { *reinterpret_cast<F4u*>(gUo + go) = F4u{du_[0], du_[1], du_[2], du_[3]}; *reinterpret_cast<F4u*>(gVo + go) = F4u{dv_[0], dv_[1], dv_[2], dv_[3]}; } \
            else { _Pragma("unroll") for (int i = 0; i < 4; i++) if ((smask >> i) & 1u) { gUo[go + i] = du_[i]; gVo[go + i] = dv_[i]; } } \
        }

    // The loader wave and the compute waves run their own copy of the step loop (same number of steps, one barrier each): the register allocation of one
    // role does not see the other's live values (two rows of pieces in flight there, two rows of coefficients here)
    if (is_loader) {
        // per piece, fixed for the launch: source pointer of row 0, LDS offset without the row part, kind (0 staging, 1 ring, -1 none), in-image mask of the 4 pixels
        // an A11 / A22 piece also leaves its reciprocals in the staging planes 5 / 6 (prd: distance to that plane, 0 = none): the step's one heavy job of
        // a compute thread -- taking over a new row pair -- is then LDS reads only.  (With the reciprocals formed by the row's owner the wave holding the
        // threads that change pairs in a step ran ~2.8 x the instructions of the others, and every step has such a wave: the barrier made its path the step time.)
        // Pieces 0 .. NCS-1 hold the staging planes' chunks (A11, A22, A12, b1, b2 -- the two that need reciprocals first), the rest the ring planes' (w, du, dv):
        // what a piece is, is known when the code is compiled, and everything that is the same for the whole wave is kept scalar (readfirstlane)
        constexpr int NCS = (5 * MAXSW + 63) / 64, NCR = (3 * MAXSW + 63) / 64, NCRCP = (2 * MAXSW + 63) / 64;
        static_assert(NCS + NCR == SS_NC, "k_sor_stream: pieces per loader lane");
        const int srow = __builtin_amdgcn_readfirstlane(lrow);
        const float* psrc[SS_NC]; int pdst[SS_NC], prd[SS_NC]; unsigned pmask[SS_NC]; bool pact[SS_NC];
        int slowbits = 0, rcpbits = 0;                            // per piece: holds du / dv chunks that stick out of the image; holds A11 / A22 chunks
        #pragma unroll
        for (int c = 0; c < SS_NC; c++) {
            const bool stg = c < NCS;
            const int id = llane + 64 * (stg ? c : c - NCS), lp = id / SW, lch = id - lp * SW, gx = ex0 + 4 * lch;
            pact[c] = id < (stg ? 5 : 3) * SW;
            const float* plane = stg ? (lp == 0 ? gA11 : lp == 1 ? gA22 : lp == 2 ? gA12 : lp == 3 ? gB1 : gB2) : (lp == 0 ? gW : lp == 1 ? gU : gV);
            psrc[c] = (pact[c] ? plane : gA11) + base + min(gx, w - 1);      // (a chunk wholly right of the image re-reads around the last pixel; inactive lanes read somewhere valid)
            // staging planes in LDS: 0 A11, 1 A12, 2 A22, 3 b1, 4 b2, 5 1 / A11, 6 1 / A22; every plane split by column parity: even columns first
            pdst[c] = (stg ? O_ST + (lp == 0 ? 0 : lp == 1 ? 2 : lp == 2 ? 1 : lp) * STP : (lp == 0 ? O_W : lp == 1 ? O_DU : O_DV)) + 2 * lch;
            pmask[c] = (gx < w ? 1u : 0u) | (gx + 1 < w ? 2u : 0u) | (gx + 2 < w ? 4u : 0u) | (gx + 3 < w ? 8u : 0u);
            prd[c] = (stg && pact[c] && lp == 0) ? 5 * STP : (stg && pact[c] && lp == 1) ? 4 * STP : 0;
            // what has to read as zero outside the image is du / dv (a neighbour's sum takes them) and the reciprocals (an outside pixel's update is then
            // exactly 0 whatever finite coefficients it reads: the row's continuation in memory, or the zeroed padding behind the planes)
            if (__builtin_amdgcn_ballot_w64(!stg && pact[c] && lp >= 1 && pmask[c] != 0xfu) != 0ull) slowbits |= 1 << c;
            if (__builtin_amdgcn_ballot_w64(prd[c] != 0) != 0ull) rcpbits |= 1 << c;
        }
        slowbits = __builtin_amdgcn_readfirstlane(slowbits); rcpbits = __builtin_amdgcn_readfirstlane(rcpbits);
        for (int T0 = -4; T0 < (h + 1) / 2 + SS_NQ + 2; T0 += 2) {
            #pragma unroll
            for (int tt = 0; tt < 2; tt++) {
                // step T: the pieces of row pair T + 1 (requested two steps ago) go to LDS, then the pieces of pair T + 3 are requested: SS_NC loads per step and loader,
                // always (rows outside the image re-read row 0 / h - 1 and are masked when parked), so that "at most SS_NC loads outstanding" means exactly
                // "the loads of two steps ago have landed".  The loads are inline assembly: the compiler's own s_waitcnt would be vmcnt(0) at every use of a
                // loaded register in this loop (it cannot count across the back edge), i.e. one full memory latency per piece instead of per step.
                const int T = T0 + tt;
                asm volatile("s_waitcnt vmcnt(%0)" :: "n"(SS_NC) : "memory");
                {
                    const int ys = 2 * (T + 1) + srow;
                    const bool park = ys >= 0 && ys <= h + 1, rowin = ys < h;       // the two rows below the image read as zero
                    const int stg_off = (ys & (SS_STG - 1)) * EWS, ring_off = (((ys % SS_RING) + SS_RING) % SS_RING) * HS;
                    #pragma unroll
                    for (int c = 0; c < SS_NC; c++) {
                        ss_f4 q = pf[tt][c];
                        asm volatile("" : "+v"(q));                                   // (uses stay behind the wait above)
                        if (!park) continue;
                        if (c < NCS) {
                            if (!rowin) continue;                                     // (nobody takes over a row below the image)
                            float* dst = lds + pdst[c] + stg_off;
                            if (pact[c]) { *reinterpret_cast<float2*>(dst) = make_float2(q.x, q.z); *reinterpret_cast<float2*>(dst + EWS / 2) = make_float2(q.y, q.w); }
                            if (c < NCRCP && ((rcpbits >> c) & 1)) {
                                const float r0 = sor_rcp(q.x), r1 = sor_rcp(q.y), r2 = sor_rcp(q.z), r3 = sor_rcp(q.w);
                                const unsigned m = pmask[c];
                                if (prd[c]) {
                                    *reinterpret_cast<float2*>(dst + prd[c]) = make_float2((m & 1u) ? r0 : 0.f, (m & 4u) ? r2 : 0.f);
                                    *reinterpret_cast<float2*>(dst + prd[c] + EWS / 2) = make_float2((m & 2u) ? r1 : 0.f, (m & 8u) ? r3 : 0.f);
                                }
                            }
                        } else {
                            float* dst = lds + pdst[c] + ring_off;
                            if (((slowbits >> c) & 1) || !rowin) {
                                const unsigned m = rowin ? pmask[c] : 0u;                // (a weight chunk is masked with its piece: nobody reads a weight outside the image)
                                if (pact[c]) { *reinterpret_cast<float2*>(dst) = make_float2((m & 1u) ? q.x : 0.f, (m & 4u) ? q.z : 0.f); *reinterpret_cast<float2*>(dst + PL) = make_float2((m & 2u) ? q.y : 0.f, (m & 8u) ? q.w : 0.f); }
                            } else if (pact[c]) { *reinterpret_cast<float2*>(dst) = make_float2(q.x, q.z); *reinterpret_cast<float2*>(dst + PL) = make_float2(q.y, q.w); }
                        }
                    }
                }
                {
                    const int yl = min(max(2 * (T + 3) + srow, 0), h - 1);
                    const size_t src_off = (size_t)yl * w;
                    #pragma unroll
                    for (int c = 0; c < SS_NC; c++) { const float* a = psrc[c] + src_off; asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(pf[tt][c]) : "v"(a) : "memory"); }
                }
                ss_lds_barrier();
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        return;
    }
    // Per-thread pipeline state, touched only when the thread changes pairs (every SS_NQ steps): the ring rows of its pair (pA, pB), of the row above (pU)
    // and below (pD), whether the pair's rows exist, and s = T - p counted up step by step
    float *pA, *pB, *pU, *pD, *pS = lds; int yS = 0; bool okA, okB, stS = false;
    #define SS_PAIR()                                                                                                              \
        {                                                                                                                          \
            const int sa_ = (2 * p) % SS_RING;                                                                                     \
            pA = lds + sa_ * HS + k2; pB = lds + (sa_ + 1) * HS + k2;        /* (2 p is even and SS_RING is: the odd row never wraps) */ \
            pU = lds + (sa_ == 0 ? SS_RING - 1 : sa_ - 1) * HS + k2; pD = lds + (sa_ + 2 == SS_RING ? 0 : sa_ + 2) * HS + k2;      \
            okA = 2 * p < h; okB = 2 * p + 1 < h;                                                                                  \
        }
    SS_PAIR()
    int sg = -4 - p;
    const int sgrp = __builtin_amdgcn_readfirstlane(g);        // (a slot group is whole waves: the colour of a step is a scalar)
    for (int T0 = -4; T0 < (h + 1) / 2 + SS_NQ + 2; T0 += 2) {
        #pragma unroll 1
        for (int tt = 0; tt < 2; tt++) {
            const int par = (tt + sgrp) & 1;
            // step T of this thread's row pair p: s = T - p.  First its odd row's half-sweep s - 1, then its even row's half-sweep s (the even row's vertical
            // neighbours in the odd row are of the colour just updated -- same thread, same columns).  Both update the column parity s & 1 = (T + g) & 1.
            if (sg == 1 && stS) SS_STORE(yS, pS)               // the odd row of the pair left in the last step (the ring keeps a finished row for two steps)
            if (sg >= 1 && okB) { if (par == 0) SS_HALF_B(0) else SS_HALF_B(1) }
            if (sg == SS_NQ) {                                  // the pair is through: the thread takes the pair SS_NQ further down (same parity)
                pS = pB; yS = 2 * p + 1; stS = okB;
                p += SS_NQ; sg = 0;
                SS_PAIR()
            }
            if (sg == 0 && okA) {
                SS_LOAD(A, 2 * p, pA)
                if (okB) SS_LOAD(B, 2 * p + 1, pB)
                else { _Pragma("unroll") for (int i = 0; i < 4; i++) B.du[i] = B.dv[i] = 0.f; }      // the row below the image reads as zero
            }
            if (sg >= 0 && okA) { if (par == 0) SS_HALF_A(0) else SS_HALF_A(1) }
            if (sg == SS_NQ - 1 && okA) SS_STORE(2 * p, pA)
            ss_lds_barrier();
            sg++;
        }
    }
    #undef SS_PAIR
    #undef SS_LOAD
    #undef SS_HALF_A
    #undef SS_HALF_B
    #undef SS_UPDATE
    #undef SS_STORE
}
// The launch: workgroup k takes the items k, k + gridDim.x, ... (item = strip + strips * image).  With as many workgroups as items (the default) a workgroup has one item;
// with FEWER (launch_sor_stream: SolverCfg::stream_wg_cap) the workgroups are persistent: they keep their place on their compute units for the whole launch instead of handing it back
// after every item -- and a place that is handed back while other kernels' small workgroups are queued at a higher stream priority comes back in pieces.
template <int MAXSW>
__global__ void __attribute__((amdgpu_flat_work_group_size(64, 512), amdgpu_waves_per_eu(4, 4))) k_sor_stream(int strips, int items, int w, int h, int SW, int HT, int IW, float omega, const float* __restrict__ gA11, const float* __restrict__ gA12,
                                                     const float* __restrict__ gA22, const float* __restrict__ gB1, const float* __restrict__ gB2,
                                                     const float* __restrict__ gW, const float* __restrict__ gU, const float* __restrict__ gV, float* __restrict__ gUo, float* __restrict__ gVo) {
    extern __shared__ float4 lds4s[];
    float* lds = reinterpret_cast<float*>(lds4s);
    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        const int image = item / strips, strip = item - image * strips;
        ss_item<MAXSW>(lds, strip, image, w, h, SW, HT, IW, omega, gA11, gA12, gA22, gB1, gB2, gW, gU, gV, gUo, gVo);
        __syncthreads();                                          // every wave is through with the item's LDS before the next item clears it
    }
}

// a launch is SS_NQ / 2 = 5 iterations of a level of at least two row pairs
static_assert(SS_NQ / 2 == 5, "sor_plan counts five iterations per launch of k_sor_stream");
bool sor_stream_fits(int h, int total) { return h >= 4 && total % (SS_NQ / 2) == 0; }
// 5 iterations of a level; the result is in P.dWu / P.dWv (swapped with their partners).  wg_cap > 0: at most that many (persistent) workgroups
int launch_sor_stream(hipStream_t s, FlowPlanes& P, int w, int h, int B, float omega, int wg_cap) {
    // the flow slices call this concurrently from their own threads: set the (idempotent) attribute once per device
    static SindPerDeviceInit attr_init;
    HIP_TRY(attr_init.run([] { return hipFuncSetAttribute((const void*)k_sor_stream<SS_MAXSW>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024); }));
    // column strips: n = fewest strips whose working width (kept columns + 12 on each cut side, a multiple of 4) fits 4 SS_MAXSW = 152 columns
    int n = 1, IW = divup(w, 4) * 4, SW = IW / 4;
    while (SW > SS_MAXSW) { n++; IW = divup(divup(w, n), 4) * 4; SW = (IW + 24) / 4; }
    const int HT = divup(5 * SW, 64) * 64, CT = 2 * HT;       // threads of one slot group (whole waves: a wave holding both groups would run both colours' code every step), compute threads; + two loader waves
    const size_t shm = ((size_t)6 * SS_RING * (2 * SS_MAXSW + 4) + (size_t)SS_NST * SS_STG * 4 * SS_MAXSW) * sizeof(float);
    const int items = n * B, wgs = (wg_cap > 0 && items > wg_cap) ? divup(items, divup(items, wg_cap)) : items;      // persistent: every workgroup the same number of items (+- 1)
    hipLaunchKernelGGL(k_sor_stream<SS_MAXSW>, dim3(wgs), dim3(CT + 128), shm, s, n, items, w, h, SW, HT, IW, omega, P.A11, P.A12, P.A22, P.b1, P.b2, P.wgt, P.dWu, P.dWv, P.dWu2, P.dWv2);
    std::swap(P.dWu, P.dWu2); std::swap(P.dWv, P.dWv2);      // column strips read each other's halo columns: not in place
    return SIND_OK;
}

}  // namespace sind
