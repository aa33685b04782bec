// pos_loss.hip -- the loss terms of the reference's MultiBoxLoss that act on the positive priors only (layers/modules/multibox_loss.py):
// losses['BIoU'] (:164-172) with losses['center'] (:450-455), and losses['T'] (track_loss, :328-351), for gfx950.  Dense forms: no boolean
// gather, no compaction of the inputs, no host synchronisation, no float atomics; every grid depends on the shapes only; sums run in double in
// a fixed order, so loss and gradients are bit-identical from run to run; outputs are written, not accumulated.  Conventions:
// include/stmask_hip.h.  pos_i = conf_t_i > 0, npos_b the positives of image b, w_i = 1 / max(npos_b, 1).
//
// Tiles: a workgroup owns 256 consecutive priors of ONE image (tiles do not straddle images): tpi = ceil(P / 256) tiles per image, B * tpi in all.
//
// Box / centerness (3 launches):
//   1 rows      one thread per prior; a thread whose prior is not positive reads nothing but conf_t.  A positive decodes its box
//               (stm_decode_one), evaluates DIoU against its ground truth in the reference's fp32 operation order, and the tile writes the
//               unweighted double sums of 1 - DIoU and of smooth_l1(c, DIoU) and its count of positives
//   2 reduce    one workgroup: per image the tiles in order, divided by max(npos_b, 1); the images in a fixed order; npos [B] is written out
//   3 adjoint   one thread per prior, from npos and the two incoming gradients: decode and DIoU are recomputed for a positive; every other row
//               of grad_loc (one 16-byte store) and grad_centerness is an exact zero, written without reading the boxes.
//
// Track loss.  With the n positives of the batch in flattened index order, s_ij = (x_i . x_j + 1) / 2 and L_ij = -log(max(s_ij, 1e-10)) for
// equal ids, -log(max(1 - s_ij, 1e-10)) otherwise:  T = alpha * sum_{i<j} w_i w_j L_ij / W,  W = sum_{i<j} w_i w_j.  n never reaches the host.
//   1 count     positives per tile
//   2 scan      one workgroup: the tiles' prefix, n, npos_b, and W = ((sum_b npos_b w_b)^2 - sum_b npos_b w_b^2) / 2 in double
//   3 index     the ordered list of positive rows and their weights (stm_block_excl_scan inside the tile)
//   4 pairs     a persistent grid of TL_G workgroups; workgroup g takes the upper-triangle pairs (bi <= bj) of 64-row blocks t = g, g + TL_G, ...
//               up to the device-side count.  The two row blocks are gathered through the index list into LDS in chunks of TL_DC = 32 columns
//               (rows are D contiguous floats: the loads run along a row and coalesce, any D, no alignment needed); a thread owns a 4 x 4
//               patch of the 64 x 64 dots (fp32 FMAs in column order); the pair terms are formed in double and added thread, wave,
//               workgroup, tile pair in a fixed order into the workgroup's own double
//   5 reduce    one workgroup adds the TL_G partials in order and scales; n < 2 gives exactly 0 (the reference: NaN)
// Adjoint (the same launches 1-3 rebuild the list: nothing is saved between forward and backward), then
//   4 zero      grad_track is cleared with 16-byte stores; track_data is not read
//   5 rows      grid (ceil(B * P / 64), ceil(D / 128)), workgroups past the device-side block count leave at once.  A workgroup owns 64
//               positive rows and a slab of 128 columns and walks ALL column blocks in order, in the manner of an attention backward: the
//               64 x 64 dots again, coef_ij = g alpha / W * w_i w_j * dL/ds / 2 (i != j) into LDS, then grad_i += coef_ij x_j with 4 x 8
//               register accumulators per thread.  No atomics; every positive row is written once.
// What bounds the tile: two 64 x 33 fp32 staging tiles (16.5 KiB; the odd pitch keeps the 16 rows that a half wave reads at one column on 16
// banks and the row-wise stores conflict-free) plus, in the adjoint, the 64 x 65 coefficients (16.3 KiB): 33 KiB, four workgroups per CU of
// 160 KiB; a wider chunk of D buys nothing (the loop is FMA-bound at 8 LDS reads per 16 FMAs) and a 128 x 128 tile would leave most CUs idle
// at the n ~ 10^3 of training.  D <= 512 bounds the recomputation of the dots over the column slabs to 4 x.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no kernel of this file uses scratch.
#include "stm_common.h"
#include "pos_index.h"

namespace {

constexpr int TL_MAX_D = 512;
constexpr int TL_BLK = 64;             // positives per row / column block
constexpr int TL_DC = 32;              // columns of track_data staged at a time
constexpr int TL_LD = TL_DC + 1;       // pitch of the staging tiles
constexpr int TL_G = 256;              // workgroups of the persistent pair grid
constexpr int TL_SLAB = 128;           // columns of grad_track per adjoint workgroup
constexpr int TL_CLD = TL_BLK + 1;     // pitch of the coefficient tile

// ------------------------------------------------------------------------------------------ DIoU
struct Diou {
    float iou, ex, ey, c2raw, c2, dx, dy, d2, q, diou;
};

// get_DIoU (:227-245) of one pair in fp32, the reference's operation order; p: the predicted box, g: its ground truth (jaccard's box_a)
__device__ __forceinline__ Diou pl_diou(const float4 p, const float4 g)
{
    Diou r;
    r.iou = stm_iou(g, p);
    const float xmax = fmaxf(fmaxf(p.x, p.z), fmaxf(g.x, g.z)), xmin = fminf(fminf(p.x, p.z), fminf(g.x, g.z));
    const float ymax = fmaxf(fmaxf(p.y, p.w), fmaxf(g.y, g.w)), ymin = fminf(fminf(p.y, p.w), fminf(g.y, g.w));
    r.ex = xmax - xmin;
    r.ey = ymax - ymin;
    r.c2raw = r.ex * r.ex + r.ey * r.ey;
    r.c2 = r.c2raw < 1e-10f ? 1e-10f : r.c2raw;
    r.dx = (p.x / 2.0f + p.z / 2.0f) - (g.x / 2.0f + g.z / 2.0f);
    r.dy = (p.y / 2.0f + p.w / 2.0f) - (g.y / 2.0f + g.w / 2.0f);
    r.d2 = r.dx * r.dx + r.dy * r.dy;
    r.q = r.d2 / r.c2;
    r.diou = r.iou - r.q;
    return r;
}

// d/d(lo, hi) of max - min over cat([lo_p, hi_p, lo_g, hi_g]): the first maximal / minimal element in that order takes the gradient (torch's
// max / min over a dimension); only the predicted box's two coordinates are returned
__device__ __forceinline__ void pl_extent_adjoint(float lo_p, float hi_p, float lo_g, float hi_g, float gext, float& glo, float& ghi)
{
    const float v[4] = {lo_p, hi_p, lo_g, hi_g};
    int imax = 0, imin = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        if (v[k] > v[imax]) imax = k;
        if (v[k] < v[imin]) imin = k;
    }
    glo = (imax == 0 ? gext : 0.0f) - (imin == 0 ? gext : 0.0f);
    ghi = (imax == 1 ? gext : 0.0f) - (imin == 1 ? gext : 0.0f);
}

__global__ __launch_bounds__(256) void box_center_rows_kernel(const float4* __restrict__ loc, const float4* __restrict__ priors,
                                                              int64_t prior_img_stride, const float4* __restrict__ gt,
                                                              const int64_t* __restrict__ conf_t, const float* __restrict__ cent,
                                                              double* __restrict__ part, unsigned* __restrict__ tilecnt, int P, int tpi)
{
    __shared__ double sd[4];
    __shared__ unsigned sc[4];
    int img, rows;
    int64_t row0;
    pl_tile(tpi, P, img, row0, rows);
    const int tid = threadIdx.x;
    const int64_t row = row0 + tid;
    const bool pos = tid < rows && conf_t[row] > 0;
    double tb = 0.0, tc = 0.0;
    if (pos) {
        const float4 p = stm_decode_one(loc[row], priors[(int64_t)img * prior_img_stride + (row - (int64_t)img * P)]);
        const Diou r = pl_diou(p, gt[row]);
        tb = (double)(1.0f - r.diou);
        if (cent) {
            const float d = cent[row] - r.diou, ad = fabsf(d);
            tc = (double)(ad < 1.0f ? 0.5f * d * d : ad - 0.5f);
        }
    }
    const unsigned long long m = __ballot(pos);
    if ((tid & 63) == 0) sc[tid >> 6] = (unsigned)__popcll(m);
    const double sb = stm_block_sum_f64(tb, sd);                    // (its barriers publish sc)
    const unsigned cnt = sc[0] + sc[1] + sc[2] + sc[3];
    const double scn = cent ? stm_block_sum_f64(tc, sd) : 0.0;
    if (tid == 0) {
        part[2 * (size_t)blockIdx.x] = sb;
        part[2 * (size_t)blockIdx.x + 1] = scn;
        tilecnt[blockIdx.x] = cnt;
    }
}

__global__ __launch_bounds__(256) void box_center_reduce_kernel(const double* __restrict__ part, const unsigned* __restrict__ tilecnt,
                                                                float* __restrict__ biou, float* __restrict__ center, int* __restrict__ npos,
                                                                int B, int tpi, double alpha_b, double alpha_c)
{
    __shared__ double sd[4];
    double ab = 0.0, ac = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) {
        unsigned cnt = 0;
        double sb = 0.0, sc = 0.0;
        for (int t = 0; t < tpi; ++t) {
            const size_t i = (size_t)b * tpi + t;
            cnt += tilecnt[i];
            sb += part[2 * i];
            sc += part[2 * i + 1];
        }
        npos[b] = (int)cnt;
        const double den = (double)(cnt > 1u ? cnt : 1u);
        ab += sb / den;
        ac += sc / den;
    }
    ab = stm_block_sum_f64(ab, sd);
    ac = stm_block_sum_f64(ac, sd);
    if (threadIdx.x == 0) {
        *biou = (float)(alpha_b * ab);
        if (center) *center = (float)(alpha_c * ac);
    }
}

__global__ __launch_bounds__(256) void box_center_backward_kernel(const float* __restrict__ g_biou, const float* __restrict__ g_center,
                                                                  const float4* __restrict__ loc, const float4* __restrict__ priors,
                                                                  int64_t prior_img_stride, const float4* __restrict__ gt,
                                                                  const int64_t* __restrict__ conf_t, const float* __restrict__ cent,
                                                                  const int* __restrict__ npos, float4* __restrict__ grad_loc,
                                                                  float* __restrict__ grad_cent, int P, int tpi, double alpha_b, double alpha_c)
{
    int img, rows;
    int64_t row0;
    pl_tile(tpi, P, img, row0, rows);
    const int tid = threadIdx.x;
    if (tid >= rows) return;
    const int64_t row = row0 + tid;
    float4 gl = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float gc = 0.0f;
    if (conf_t[row] > 0) {
        const int np = npos[img];
        const double w = 1.0 / (double)(np > 1 ? np : 1);                  // the incoming gradient, alpha and w_i: one rounding
        const float sB = g_biou ? (float)((double)g_biou[0] * alpha_b * w) : 0.0f;
        const float sC = (g_center && cent) ? (float)((double)g_center[0] * alpha_c * w) : 0.0f;
        const float4 l = loc[row], pr = priors[(int64_t)img * prior_img_stride + (row - (int64_t)img * P)], g = gt[row];
        const float4 p = stm_decode_one(l, pr);
        const Diou r = pl_diou(p, g);
        float gD = -sB;                                      // d(1 - DIoU)
        if (cent) {                                          // smooth-L1's target is NOT detached in the reference
            const float d = cent[row] - r.diou;
            const float sl = fabsf(d) < 1.0f ? d : (d > 0.0f ? 1.0f : -1.0f);
            gc = sC * sl;
            gD = gD - gc;
        }
        const float gq = -gD;                                // DIoU = IoU - d2 / c2
        const float gd2 = gq / r.c2;
        const float gc2 = r.c2raw < 1e-10f ? 0.0f : -(gq * r.q) / r.c2;   // the clamp passes nothing where it cut
        float4 gp, ga;
        stm_iou_adjoint(g, p, gD, ga, gp);
        float glo, ghi;
        pl_extent_adjoint(p.x, p.z, g.x, g.z, gc2 * 2.0f * r.ex, glo, ghi);
        const float gdx = gd2 * 2.0f * r.dx / 2.0f, gdy = gd2 * 2.0f * r.dy / 2.0f;
        gp.x += glo + gdx;
        gp.z += ghi + gdx;
        pl_extent_adjoint(p.y, p.w, g.y, g.w, gc2 * 2.0f * r.ey, glo, ghi);
        gp.y += glo + gdy;
        gp.w += ghi + gdy;
        float4 gpr;
        stm_decode_one_adjoint(gp, l, pr, gl, gpr);
    }
    grad_loc[row] = gl;
    if (grad_cent) grad_cent[row] = gc;
}

// ------------------------------------------------------------------------------------------ track loss
// the list's workspace (pos_index.h) with the TL_G partial doubles of the pairs kernel as its extra block
PosLayout track_layout(int B, int P) { return pos_layout(B, P, 2 * (size_t)TL_G); }

// Rows blk * 64 .. + 63 of the list, columns k0 .. k0 + TL_DC - 1 of track_data -> tile[64][TL_LD]; rows past n and columns past D are zeros.
// A thread's 8 loads run along rows (32 consecutive lanes, 32 consecutive floats).
__device__ __forceinline__ void tl_stage(float* __restrict__ tile, const float* __restrict__ x, const int* __restrict__ rows, int k0, int D)
{
    const int k = threadIdx.x & (TL_DC - 1), r0 = threadIdx.x >> 5;
#pragma unroll
    for (int j = 0; j < TL_BLK / 8; ++j) {
        const int r = r0 + 8 * j;
        const int src = rows[r];
        tile[r * TL_LD + k] = (src >= 0 && k0 + k < D) ? x[(int64_t)src * D + k0 + k] : 0.0f;
    }
}

// the list's rows, ids and weights of block blk into LDS (threads 0..63); a slot past n has row -1 and weight 0
__device__ __forceinline__ void tl_block_meta(int blk, unsigned n, const int* __restrict__ idx, const float* __restrict__ wts,
                                              const int64_t* __restrict__ ids_t, int* srow, int64_t* sid, float* sw, int t)
{
    const unsigned gi = (unsigned)blk * TL_BLK + (unsigned)t;
    const bool live = gi < n;
    const int row = live ? idx[gi] : -1;
    srow[t] = row;
    sid[t] = live ? ids_t[row] : 0;
    sw[t] = live ? wts[gi] : 0.0f;
}

// the 4 x 4 patch (rows ty + 16 a, columns tx + 16 b) of A . B^T over the staged chunk, added onto acc in column order
__device__ __forceinline__ void tl_dots(const float* __restrict__ ta, const float* __restrict__ tb, int ty, int tx, float (&acc)[4][4])
{
#pragma unroll 4
    for (int k = 0; k < TL_DC; ++k) {
        float av[4], bv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) av[a] = ta[(ty + 16 * a) * TL_LD + k];
#pragma unroll
        for (int b = 0; b < 4; ++b) bv[b] = tb[(tx + 16 * b) * TL_LD + k];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = fmaf(av[a], bv[b], acc[a][b]);
    }
}

__global__ __launch_bounds__(256) void track_pairs_kernel(const float* __restrict__ x, const int64_t* __restrict__ ids_t,
                                                          const unsigned* __restrict__ meta, const int* __restrict__ idx,
                                                          const float* __restrict__ wts, double* __restrict__ part, int D)
{
    __shared__ float ta[TL_BLK * TL_LD], tb[TL_BLK * TL_LD];
    __shared__ int rowa[TL_BLK], rowb[TL_BLK];
    __shared__ int64_t ida[TL_BLK], idb[TL_BLK];
    __shared__ float wa[TL_BLK], wb[TL_BLK];
    __shared__ double sd[4];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const unsigned n = meta[TM_N];
    const unsigned nb = (n + TL_BLK - 1) / TL_BLK;
    double total = 0.0;                                      // (thread 0's copy is the workgroup's sum)
    // pair t of the upper triangle, row-major: row bi holds the nb - bi pairs (bi, bi), (bi, bi + 1), ...
    unsigned bi = 0;
    unsigned long long off = blockIdx.x;
    while (bi < nb) {
        while (bi < nb && off >= (unsigned long long)(nb - bi)) {
            off -= nb - bi;
            ++bi;
        }
        if (bi >= nb) break;
        const unsigned bj = bi + (unsigned)off;
        __syncthreads();                                     // the previous pair's readers are done with the block tables
        if (tid < TL_BLK) tl_block_meta((int)bi, n, idx, wts, ids_t, rowa, ida, wa, tid);
        else if (tid < 2 * TL_BLK) tl_block_meta((int)bj, n, idx, wts, ids_t, rowb, idb, wb, tid - TL_BLK);
        float acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = 0.0f;
        for (int k0 = 0; k0 < D; k0 += TL_DC) {
            __syncthreads();                                 // the tables are written; the previous chunk is consumed
            tl_stage(ta, x, rowa, k0, D);
            tl_stage(tb, x, rowb, k0, D);
            __syncthreads();
            tl_dots(ta, tb, ty, tx, acc);
        }
        double sum = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int i = ty + 16 * a, j = tx + 16 * b;
                const unsigned gi = bi * TL_BLK + i, gj = bj * TL_BLK + j;
                if (gi < gj && gj < n) {
                    const double s = ((double)acc[a][b] + 1.0) / 2.0;
                    const double v = ida[i] == idb[j] ? s : 1.0 - s;
                    sum += (double)wa[i] * (double)wb[j] * -log(v < 1e-10 ? 1e-10 : v);
                }
            }
        total += stm_block_sum_f64(sum, sd);
        off += TL_G;
    }
    if (tid == 0) part[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void track_reduce_kernel(const double* __restrict__ part, const unsigned* __restrict__ meta,
                                                           float* __restrict__ loss, double alpha)
{
    __shared__ double sd[4];
    static_assert(TL_G == 256, "one partial per thread");
    const double s = stm_block_sum_f64(part[threadIdx.x], sd);
    if (threadIdx.x == 0) {
        const double W = *reinterpret_cast<const double*>(meta + TM_W);
        *loss = meta[TM_N] >= 2u ? (float)(alpha * s / W) : 0.0f;
    }
}

__global__ __launch_bounds__(256) void track_zero_kernel(float* __restrict__ p, int64_t n)
{
    const int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e + 3 < n) {
        *reinterpret_cast<float4*>(p + e) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    } else {
        for (int j = 0; e + j < n; ++j) p[e + j] = 0.0f;
    }
}

__global__ __launch_bounds__(256) void track_backward_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                             const int64_t* __restrict__ ids_t, const unsigned* __restrict__ meta,
                                                             const int* __restrict__ idx, const float* __restrict__ wts,
                                                             float* __restrict__ gx, int D, double alpha)
{
    __shared__ float ta[TL_BLK * TL_LD], tb[TL_BLK * TL_LD];
    __shared__ float coef[TL_BLK * TL_CLD];
    __shared__ int rowa[TL_BLK], rowb[TL_BLK];
    __shared__ int64_t ida[TL_BLK], idb[TL_BLK];
    __shared__ float wa[TL_BLK], wb[TL_BLK];
    const unsigned n = meta[TM_N];
    const unsigned nb = (n + TL_BLK - 1) / TL_BLK;
    const unsigned bi = blockIdx.x;
    if (bi >= nb) return;                                    // workgroup-uniform
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int d0 = blockIdx.y * TL_SLAB;
    const double W = *reinterpret_cast<const double*>(meta + TM_W);
    const double scale = n >= 2u ? (double)g[0] * alpha / W * 0.5 : 0.0;
    if (tid < TL_BLK) tl_block_meta((int)bi, n, idx, wts, ids_t, rowa, ida, wa, tid);
    float gacc[4][8];                                        // rows ty + 16 a, columns d0 + 32 c + tx + 16 h at [a][2 c + h]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 8; ++c) gacc[a][c] = 0.0f;
    for (unsigned bj = 0; bj < nb; ++bj) {
        __syncthreads();                                     // the previous column block's readers are done
        if (tid < TL_BLK) tl_block_meta((int)bj, n, idx, wts, ids_t, rowb, idb, wb, tid);
        float acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = 0.0f;
        for (int k0 = 0; k0 < D; k0 += TL_DC) {
            __syncthreads();
            tl_stage(ta, x, rowa, k0, D);
            tl_stage(tb, x, rowb, k0, D);
            __syncthreads();
            tl_dots(ta, tb, ty, tx, acc);
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int i = ty + 16 * a, j = tx + 16 * b;
                const unsigned gi = bi * TL_BLK + i, gj = bj * TL_BLK + j;
                float c = 0.0f;
                if (gi != gj && gi < n && gj < n) {
                    const double s = ((double)acc[a][b] + 1.0) / 2.0;
                    double dl;                               // dL/ds; exactly 0 where the clamp cut
                    if (ida[i] == idb[j]) dl = s > 1e-10 ? -1.0 / s : 0.0;
                    else dl = 1.0 - s > 1e-10 ? 1.0 / (1.0 - s) : 0.0;
                    c = (float)(scale * ((double)wa[i] * (double)wb[j]) * dl);
                }
                coef[i * TL_CLD + j] = c;
            }
#pragma unroll
        for (int c = 0; c < TL_SLAB / TL_DC; ++c) {
            const int k0 = d0 + c * TL_DC;
            if (k0 >= D) break;                              // workgroup-uniform
            __syncthreads();                                 // coef is written; tb's previous readers are done
            tl_stage(tb, x, rowb, k0, D);
            __syncthreads();
            for (int j = 0; j < TL_BLK; ++j) {
                const float x0 = tb[j * TL_LD + tx], x1 = tb[j * TL_LD + tx + 16];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const float cv = coef[(ty + 16 * a) * TL_CLD + j];
                    gacc[a][2 * c] = fmaf(cv, x0, gacc[a][2 * c]);
                    gacc[a][2 * c + 1] = fmaf(cv, x1, gacc[a][2 * c + 1]);
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int row = rowa[ty + 16 * a];
        if (row < 0) continue;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int d = d0 + (c >> 1) * TL_DC + tx + 16 * (c & 1);
            if (d < D) gx[(int64_t)row * D + d] = gacc[a][c];
        }
    }
}

int track_check(const char* who, int B, int P, int D)
{
    const int rc = pos_check(who, B, P);
    if (rc != STM_OK) return rc;
    STM_REQUIRE(D >= 1 && D <= TL_MAX_D, STM_EUNSUPPORTED, "%s: D=%d is outside [1, %d]", who, D, TL_MAX_D);
    return STM_OK;
}

// launches 1-3 of the track loss: the ordered list of positives, their weights, n and W in the workspace
int track_index(const int64_t* conf_t, int B, int P, unsigned* ws, const PosLayout& L, hipStream_t st)
{
    return pos_list(conf_t, true, nullptr, 0, B, P, ws, L, st);
}

}  // namespace

extern "C" size_t stm_box_center_workspace_bytes(int B, int P)
{
    if (B <= 0 || P <= 0 || (int64_t)B * P > PL_MAX_N) return 64;
    const size_t nT = (size_t)B * stm_cdiv(P, PL_TILE);
    return nT * (2 * sizeof(double) + sizeof(unsigned)) + 64;
}

extern "C" int stm_box_center_loss_f32(const float* loc, const float* priors, int priors_per_image, const float* gt_boxes, const int64_t* conf_t,
                                       const float* centerness, float* biou, float* center, int* npos, int B, int P, double bboxiou_alpha,
                                       double center_alpha, void* workspace, size_t workspace_bytes, stm_stream_t stream)
{
    const char* who = "stm_box_center_loss_f32";
    const int rc = pos_check(who, B, P);
    if (rc != STM_OK) return rc;
    STM_REQUIRE(priors_per_image == 0 || priors_per_image == 1, STM_EINVAL, "%s: priors_per_image=%d", who, priors_per_image);
    STM_REQUIRE(loc && priors && gt_boxes && conf_t && biou && npos, STM_ENULL, "%s: loc/priors/gt_boxes/conf_t/biou/npos must be non-NULL", who);
    STM_REQUIRE((centerness != nullptr) == (center != nullptr), STM_ENULL, "%s: centerness and center go together", who);
    STM_REQUIRE(workspace && workspace_bytes >= stm_box_center_workspace_bytes(B, P), STM_EWORKSPACE, "%s: workspace too small", who);
    STM_REQUIRE((uintptr_t)loc % 16 == 0 && (uintptr_t)priors % 16 == 0 && (uintptr_t)gt_boxes % 16 == 0 && (uintptr_t)workspace % 8 == 0,
                STM_EINVAL, "%s: loc, priors and gt_boxes must be 16-byte and the workspace 8-byte aligned", who);
    const int tpi = stm_cdiv(P, PL_TILE), nT = B * tpi;
    double* part = reinterpret_cast<double*>(workspace);
    unsigned* tilecnt = reinterpret_cast<unsigned*>(part + 2 * (size_t)nT);
    hipStream_t st = stm_hs(stream);
    hipLaunchKernelGGL(box_center_rows_kernel, dim3(nT), dim3(256), 0, st, reinterpret_cast<const float4*>(loc),
                       reinterpret_cast<const float4*>(priors), (int64_t)(priors_per_image ? P : 0), reinterpret_cast<const float4*>(gt_boxes),
                       conf_t, centerness, part, tilecnt, P, tpi);
    STM_CHECK_LAUNCH("box_center_rows_kernel");
    hipLaunchKernelGGL(box_center_reduce_kernel, dim3(1), dim3(256), 0, st, part, tilecnt, biou, center, npos, B, tpi, bboxiou_alpha, center_alpha);
    STM_CHECK_LAUNCH("box_center_reduce_kernel");
    return STM_OK;
}

extern "C" int stm_box_center_loss_backward_f32(const float* grad_biou, const float* grad_center, const float* loc, const float* priors,
                                                int priors_per_image, const float* gt_boxes, const int64_t* conf_t, const float* centerness,
                                                const int* npos, float* grad_loc, float* grad_centerness, int B, int P, double bboxiou_alpha,
                                                double center_alpha, stm_stream_t stream)
{
    const char* who = "stm_box_center_loss_backward_f32";
    const int rc = pos_check(who, B, P);
    if (rc != STM_OK) return rc;
    STM_REQUIRE(priors_per_image == 0 || priors_per_image == 1, STM_EINVAL, "%s: priors_per_image=%d", who, priors_per_image);
    STM_REQUIRE(loc && priors && gt_boxes && conf_t && npos && grad_loc, STM_ENULL, "%s: loc/priors/gt_boxes/conf_t/npos/grad_loc must be non-NULL",
                who);
    STM_REQUIRE(centerness || !grad_centerness, STM_ENULL, "%s: grad_centerness without centerness", who);
    STM_REQUIRE((uintptr_t)loc % 16 == 0 && (uintptr_t)priors % 16 == 0 && (uintptr_t)gt_boxes % 16 == 0 && (uintptr_t)grad_loc % 16 == 0,
                STM_EINVAL, "%s: loc, priors, gt_boxes and grad_loc must be 16-byte aligned", who);
    const int tpi = stm_cdiv(P, PL_TILE), nT = B * tpi;
    hipLaunchKernelGGL(box_center_backward_kernel, dim3(nT), dim3(256), 0, stm_hs(stream), grad_biou, grad_center,
                       reinterpret_cast<const float4*>(loc), reinterpret_cast<const float4*>(priors), (int64_t)(priors_per_image ? P : 0),
                       reinterpret_cast<const float4*>(gt_boxes), conf_t, centerness, npos, reinterpret_cast<float4*>(grad_loc), grad_centerness,
                       P, tpi, bboxiou_alpha, center_alpha);
    STM_CHECK_LAUNCH("box_center_backward_kernel");
    return STM_OK;
}

extern "C" size_t stm_track_loss_workspace_bytes(int B, int P, int D)
{
    (void)D;
    if (B <= 0 || P <= 0 || (int64_t)B * P > PL_MAX_N) return 64;
    return track_layout(B, P).words * sizeof(unsigned) + 64;
}

extern "C" int stm_track_loss_f32(const float* track, const int64_t* conf_t, const int64_t* ids_t, float* loss, int B, int P, int D,
                                  double track_alpha, void* workspace, size_t workspace_bytes, stm_stream_t stream)
{
    const char* who = "stm_track_loss_f32";
    const int rc = track_check(who, B, P, D);
    if (rc != STM_OK) return rc;
    STM_REQUIRE(track && conf_t && ids_t && loss, STM_ENULL, "%s: track/conf_t/ids_t/loss must be non-NULL", who);
    STM_REQUIRE(workspace && workspace_bytes >= stm_track_loss_workspace_bytes(B, P, D), STM_EWORKSPACE, "%s: workspace too small", who);
    STM_REQUIRE((uintptr_t)workspace % 8 == 0, STM_EINVAL, "%s: the workspace must be 8-byte aligned", who);
    const PosLayout L = track_layout(B, P);
    unsigned* ws = reinterpret_cast<unsigned*>(workspace);
    hipStream_t st = stm_hs(stream);
    const int ri = track_index(conf_t, B, P, ws, L, st);
    if (ri != STM_OK) return ri;
    double* part = reinterpret_cast<double*>(ws + L.extra);
    hipLaunchKernelGGL(track_pairs_kernel, dim3(TL_G), dim3(256), 0, st, track, ids_t, ws + L.meta, reinterpret_cast<const int*>(ws + L.idx),
                       reinterpret_cast<const float*>(ws + L.wts), part, D);
    STM_CHECK_LAUNCH("track_pairs_kernel");
    hipLaunchKernelGGL(track_reduce_kernel, dim3(1), dim3(256), 0, st, part, ws + L.meta, loss, track_alpha);
    STM_CHECK_LAUNCH("track_reduce_kernel");
    return STM_OK;
}

extern "C" int stm_track_loss_backward_f32(const float* grad_loss, const float* track, const int64_t* conf_t, const int64_t* ids_t,
                                           float* grad_track, int B, int P, int D, double track_alpha, void* workspace, size_t workspace_bytes,
                                           stm_stream_t stream)
{
    const char* who = "stm_track_loss_backward_f32";
    const int rc = track_check(who, B, P, D);
    if (rc != STM_OK) return rc;
    STM_REQUIRE(grad_loss && track && conf_t && ids_t && grad_track, STM_ENULL, "%s: grad_loss/track/conf_t/ids_t/grad_track must be non-NULL", who);
    STM_REQUIRE(workspace && workspace_bytes >= stm_track_loss_workspace_bytes(B, P, D), STM_EWORKSPACE, "%s: workspace too small", who);
    STM_REQUIRE((uintptr_t)workspace % 8 == 0 && (uintptr_t)grad_track % 16 == 0, STM_EINVAL,
                "%s: the workspace must be 8-byte and grad_track 16-byte aligned", who);
    const PosLayout L = track_layout(B, P);
    unsigned* ws = reinterpret_cast<unsigned*>(workspace);
    hipStream_t st = stm_hs(stream);
    const int ri = track_index(conf_t, B, P, ws, L, st);
    if (ri != STM_OK) return ri;
    const int64_t total = (int64_t)B * P * D;
    hipLaunchKernelGGL(track_zero_kernel, dim3(stm_cdiv(total, 1024)), dim3(256), 0, st, grad_track, total);
    STM_CHECK_LAUNCH("track_zero_kernel");
    hipLaunchKernelGGL(track_backward_kernel, dim3(stm_cdiv((int64_t)B * P, TL_BLK), stm_cdiv(D, TL_SLAB)), dim3(256), 0, st, grad_loss, track, ids_t,
                       ws + L.meta, reinterpret_cast<const int*>(ws + L.idx), reinterpret_cast<const float*>(ws + L.wts), grad_track, D, track_alpha);
    STM_CHECK_LAUNCH("track_backward_kernel");
    return STM_OK;
}
