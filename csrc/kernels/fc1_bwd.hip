// North-star CNN backward on gfx950, first kernel (bf16 MFMA, fp32 accumulate).
//
//   fc1_bwd    : three block roles in one launch
//                  dW1 tiles : gW1[n][k] = sum_b dh[b][n] * pool[b][k]   (K = batch; the
//                              pool tile is staged in LDS and read transposed with
//                              ds_read_b64_tr_b16 as the MFMA B operand)
//                  dX tiles  : dpool[b][k] = sum_n dh[b][n] * W1[n][k]   (W1^T bf16 copy
//                              written by the optimizer kernel)
//                  1 block   : fixed-order reduction of the head slabs -> fc2 W/b and fc1
//                              bias gradients + train metrics
//                After this kernel gradient bucket 0 (fc2 + fc1) is complete.
// Compiled with the max-ilp machine scheduler (build.py FILE_FLAGS): in-step 11.4 -> 10.8 us
// at B = 256.
#include "cnn_common.h"
#include "optim_common.h"

namespace {

using namespace cnn;

// diagnostic stamps (PDM_STAMPS builds; tools/stamps_fc.py, reader "fc1_bwd"): dX tile t ->
// row t, slots 0-3; dW tile b -> row b, slots 8-13
#ifdef PDM_STAMPS
#define FC_STAMP(row, slot)                                                         \
  do {                                                                              \
    if (threadIdx.x == 0 && (row) < 256)                                            \
      pdm_stamps[(row) * 16 + (slot)] = __builtin_amdgcn_s_memtime();              \
  } while (0)
#else
#define FC_STAMP(row, slot) do { } while (0)
#endif
// dW tile: 64 feature columns x 64 * DW_MT hidden rows (each of the 4 waves owns DW_MT 16-row
// m-tiles).  DW_MT = 1 splits the 128 hidden rows over two workgroups (288 tiles): half the
// MFMA work and half the fused update's epilogue per workgroup, twice the workgroups.
#ifndef PDM_DW_MT
#define PDM_DW_MT 1
#endif
constexpr int DW_MT = PDM_DW_MT;
static_assert(DW_MT == 1 || DW_MT == 2, "dW tile: 64 or 128 hidden rows");
constexpr int DW_FT = FEAT / 64;                      // 144 feature tiles
constexpr int DW_TILES = DW_FT * (2 / DW_MT);         // 144 or 288
constexpr int DWC = 128;             // dW1 batch rows staged per LDS round
constexpr int DX_COLS = 384;         // dX tile: 32 batch rows x 384 features per workgroup
constexpr int DX_TILES = FEAT / DX_COLS;   // 24 = 8 XCDs x 3
constexpr int DX_FT = DX_COLS / 64;        // 16-feature sub-tiles per wave (6)
constexpr int NXCD = 8;              // MI355X: workgroups are dealt round-robin to 8 XCDs
static_assert(DX_TILES % NXCD == 0 && DW_TILES % NXCD == 0, "XCD-aware tile mapping");
constexpr int HR_BLOCKS = (HEAD_SLAB + 63) / 64;   // head-slab reduction workgroups (23)

// [rows][128 B] pool tile.  A transposed read's 32-lane half touches rows {0-3, 8-11} (+4)
// of a 16-row block at one 32-B column chunk each: rows of equal parity share banks, so the
// chunk is XORed with row bits 1 and 3 -> the 8 chunks cover all 64 banks once
// (tools/lds_bank_model.py; the bit-3-only swizzle was 2 passes per read)
__device__ __forceinline__ int tile_off(int row, int byte) {
  return row * 128 + (byte ^ ((((row >> 1) & 1) | (((row >> 3) & 1) << 1)) << 5));
}

// Two waves per SIMD, i.e. two workgroups per CU (<= 256 registers per lane; 162 VGPRs, no
// spill): the 503 workgroups at B = 256 (288 dW + 192 dX + 23 head-slab) run in one round
// instead of two.  fc1_bwd 10.0 -> 9.6 us, the B = 256 step 54.9 -> 53.9 us (interleaved A/B,
// profiles/r5/fc1bwd_wpe2).
__global__ __launch_bounds__(256, 2) void fc1_bwd_kernel(
    const bf16* __restrict__ dh, const bf16* __restrict__ dht, int ldt,
    const bf16* __restrict__ pool, const bf16* __restrict__ wf1t, int B, float* __restrict__ gwf1,
    bf16* __restrict__ dpool, const float* __restrict__ head_slab, int head_blocks,
    float* __restrict__ gwf2, float* __restrict__ gbf2, float* __restrict__ gbf1,
    double* __restrict__ metrics, int bid_offset, const FcUpdate fcu) {
  // [0, 16 KB): the pool tile, then the fused update's bf16 W1 fragments; [16 KB, 32 KB):
  // the fused update's W1^T fragments (double-buffered W1^T only)
  __shared__ __attribute__((aligned(16))) char tile[2 * DWC * 128];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i16 = lane & 15, q = i16 >> 2, pq = i16 & 3;
  const int nd = (ldt / 32) * DX_TILES;
  const int bid = blockIdx.x + bid_offset;

  if (bid < DW_TILES) {
    // ---- dW1 tile: 64 * DW_MT hidden rows (from n0) x 64 feature columns, K = batch ----
    // The batch is consumed in chunks of DWC rows: the whole chunk (pool rows and the
    // dh^T A fragments) is loaded with every load in flight at once, and the next chunk's
    // loads are issued before the current chunk's MFMAs.  The two hidden halves of a
    // feature tile (DW_MT = 1) are DW_FT workgroups apart: the same XCD, one L2 copy of the
    // pool tile they both read.
    const int k0 = (bid % DW_FT) * 64, n0 = (bid / DW_FT) * 64 * DW_MT;
    FC_STAMP(bid, 8);
    f32x4 acc[DW_MT][4];
#pragma unroll
    for (int i = 0; i < DW_MT; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int srow = tid >> 3, sch = tid & 7;
    uint4 pv[DWC / 32];
    bf16x8 a[DW_MT][DWC / 32];
    auto load_chunk = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
      for (int j = 0; j < DWC / 32; ++j) {
        const int row = c0 + srow + 32 * j;
        // clamped load + select: rows past B are zero (their dh rows are zero too, but
        // stale pool memory could hold non-finite bit patterns)
        const uint4 v = *reinterpret_cast<const uint4*>(pool + (int64_t)min(row, B - 1) * FEAT +
                                                        k0 + sch * 8);
        pv[j] = row < B ? v : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int mt = 0; mt < DW_MT; ++mt)
#pragma unroll
        for (int kk = 0; kk < DWC / 32; ++kk)
          a[mt][kk] = *reinterpret_cast<const bf16x8*>(   // fragment-major dh^T (frag_pos)
              dht + ((int64_t)((n0 / 16 + wave * DW_MT + mt) * (ldt / 32) +
                               (min(c0 + 32 * kk, ldt - 32) >> 5)) * 64 + lane) * 8);
    };
    load_chunk(0);
    // fused update (fcu.kind >= 0): this tile's fp32 weights and momentum, issued behind the
    // first chunk so they have landed by the epilogue
    // (with the learning rate and step count: loaded in the epilogue they were one more
    // memory round trip on its critical path)
    float fpv[DW_MT][4][4], fmv[DW_MT][4][4];
    double fc_lr = 0.0;
    int64_t fc_t = 0;
    if (fcu.kind >= 0) {
      fc_lr = *fcu.lr;
      fc_t = *fcu.step;
#pragma unroll
      for (int mt = 0; mt < DW_MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) {
            const int64_t q = (int64_t)(n0 + wave * 16 * DW_MT + mt * 16 + 4 * g + r) * FEAT + k0 +
                              16 * nt + i16;
            fpv[mt][r][nt] = fcu.p[q];
            fmv[mt][r][nt] = fcu.m[q];
          }
    }
    for (int c0 = 0; c0 < ldt; c0 += DWC) {
      __syncthreads();   // previous chunk's tile reads are done
#pragma unroll
      for (int j = 0; j < DWC / 32; ++j)
        *reinterpret_cast<uint4*>(tile + tile_off(srow + 32 * j, sch * 16)) = pv[j];
      bf16x8 ac[DW_MT][DWC / 32];
#pragma unroll
      for (int mt = 0; mt < DW_MT; ++mt)
#pragma unroll
        for (int kk = 0; kk < DWC / 32; ++kk) ac[mt][kk] = a[mt][kk];
      __syncthreads();
      FC_STAMP(bid, c0 == 0 ? 9 : 10);   // chunk landed in LDS
      if (c0 + DWC < ldt) load_chunk(c0 + DWC);
      __builtin_amdgcn_sched_barrier(0);   // next chunk's loads stay ahead of this chunk's MFMAs
      const int nk = min(DWC / 32, (ldt - c0) / 32);
#pragma unroll
      for (int kk = 0; kk < DWC / 32; ++kk) {
        if (kk < nk) {
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) {
            const s16x4 lo = lds_tr16(tile + tile_off(32 * kk + 8 * g + q, 32 * nt + 8 * pq));
            const s16x4 hi = lds_tr16(tile + tile_off(32 * kk + 8 * g + 4 + q, 32 * nt + 8 * pq));
            const bf16x8 bv = cat_tr(lo, hi);
#pragma unroll
            for (int mt = 0; mt < DW_MT; ++mt)
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ac[mt][kk], bv, acc[mt][nt], 0, 0, 0);
          }
        }
      }
    }
    FC_STAMP(bid, 11);
    if (fcu.kind < 0 || fcu.store_grad) {
#pragma unroll
      for (int mt = 0; mt < DW_MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = n0 + wave * 16 * DW_MT + mt * 16 + 4 * g + r;
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) st_ho<2>(&gwf1[(int64_t)n * FEAT + k0 + 16 * nt + i16], acc[mt][nt][r]);
        }
    }
    if (fcu.kind >= 0) {
      // world size 1 (kernels.h FcUpdate): the SGD-momentum update of this tile, from the
      // gradient still in registers; writes the fp32 weight, the momentum and the bf16 [n][k]
      // copy (the transposed copy, which this launch's dX tiles are reading, is re-derived
      // by the optimizer launch).  Same op order as the optimizer kernel: same bits.
      using namespace optim_detail;
      const Hyper h = make_hyper<OPT_SGD>(fcu, fc_lr, fc_t);
      // the bf16 copy is fragment-major (fc1_fwd's B operand, kernels.h frag_pos): this tile
      // is 4 DW_MT n-tiles x 2 k-steps of 1-KB blocks, assembled in LDS and stored as 16-B
      // chunks
      __syncthreads();   // every wave's last reads of the pool tile are done
      bf16* fr = reinterpret_cast<bf16*>(tile);
      // W1^T fragments of this tile (kernels.h shadow_t_pos, m = feature, k = hidden): for
      // each of the 4 16-feature m-frags, the 2 DW_MT 32-row k-frags of this tile, 1 KB each
      // (one contiguous range per m-frag); a lane's 4 rows r are 4 consecutive bf16 (one 8-B
      // store, 512 B contiguous per wave store)
      bf16* frt = reinterpret_cast<bf16*>(tile + DWC * 128);
#pragma unroll
      for (int mt = 0; mt < DW_MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          bf16 pt[4];
          const int nl0 = wave * 16 * DW_MT + mt * 16 + 4 * g;   // tile-local row of r = 0
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int nl = nl0 + r, kl = 16 * nt + i16;
            const int64_t q = (int64_t)(n0 + nl) * FEAT + k0 + kl;
            float m = fmv[mt][r][nt], v = 0.f;
            const float p = update<OPT_SGD>(fpv[mt][r][nt], acc[mt][nt][r], m, v, h, fcu.grad_scale);
            st_ho<2>(&fcu.p[q], p);
            st_ho<2>(&fcu.m[q], m);
            pt[r] = to_bf16(p);
            fr[(((nl >> 4) * 2 + (kl >> 5)) * 64 + ((kl >> 3) & 3) * 16 + (nl & 15)) * 8 + (kl & 7)] = pt[r];
          }
          if (fcu.shadow_t_next != nullptr)
            *reinterpret_cast<bf16x4*>(frt + (((nt * (2 * DW_MT) + (nl0 >> 5)) * 64 +
                                               (((nl0 >> 4) & 1) * 2 + (g >> 1)) * 16 + i16) * 8 +
                                              (g & 1) * 4)) = bf16x4{pt[0], pt[1], pt[2], pt[3]};
        }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 2 * DW_MT; ++u) {
        const int c = tid + 256 * u, blk = c >> 6;   // blk = local n-tile * 2 + k-step
        st_ho<2>(reinterpret_cast<uint4*>(fcu.shadow + ((int64_t)((n0 / 16 + (blk >> 1)) * (FEAT / 32) +
                                                                   (k0 >> 5) + (blk & 1)) * 64 + (c & 63)) * 8),
                 reinterpret_cast<const uint4*>(fr)[c]);
      }
      if (fcu.shadow_t_next != nullptr) {
        // local block lb = m-frag * 2 DW_MT + local k-frag -> global block
        // (k0 / 16 + m-frag) * (HID / 32) + n0 / 32 + local k-frag, 64 uint4 each
#pragma unroll
        for (int u = 0; u < 2 * DW_MT; ++u) {
          const int c = tid + 256 * u, lb = c >> 6;
          const int64_t gb = (int64_t)(k0 / 16 + lb / (2 * DW_MT)) * (HID / 32) + n0 / 32 +
                             lb % (2 * DW_MT);
          st_ho<2>(reinterpret_cast<uint4*>(fcu.shadow_t_next) + gb * 64 + (c & 63),
                   reinterpret_cast<const uint4*>(frt)[c]);
        }
      }
    }
    FC_STAMP(bid, 13);
    return;
  }

  if (bid < DW_TILES + nd) {
    // ---- dX tile: 32 batch rows x 384 features, K = 128 hidden ----
    // dpool[b][f] = dh[b][:] . W1^T[f][:] (A = dh, B = W1^T fragments): a lane holds 4 rows
    // of one feature, so a wave's store covers 4 rows x 32 B.  (The transposed product with
    // one 8-byte store per lane spread each store over 16 rows: 0.5 us slower.)  Each wave
    // owns 96 features (6 sub-tiles) x 32 rows with every operand load (24 W1^T + 8 dh
    // fragments) issued up front: at B = 256 the 192 tiles are one round of workgroups, each
    // a single load burst (the earlier 576 tiles of 128 features ran ~2.25 latency-bound
    // rounds per CU).  XCD-aware: workgroup t runs on XCD t % 8 (DW_TILES is a multiple of
    // 8), and every XCD owns 1/8 of the feature range, so each XCD's L2 holds only its 1/8
    // of W1^T.
    const int t = bid - DW_TILES;
    FC_STAMP(t, 0);
    constexpr int TPX = DX_TILES / NXCD;                 // feature tiles per XCD
    const int xcd = t % NXCD, loc = t / NXCD;
    const int b0 = (loc / TPX) * 32;
    const int f0 = (xcd * TPX + loc % TPX) * DX_COLS + wave * (16 * DX_FT);
    bf16x8 wa[DX_FT][HID / 32], hb[2][HID / 32];
#pragma unroll
    for (int ks = 0; ks < HID / 32; ++ks) {
#pragma unroll
      for (int bt = 0; bt < 2; ++bt)
        hb[bt][ks] = *reinterpret_cast<const bf16x8*>(
            dh + ((int64_t)(((b0 >> 4) + bt) * (HID / 32) + ks) * 64 + lane) * 8);   // frag_pos
#pragma unroll
      for (int ft = 0; ft < DX_FT; ++ft)
        wa[ft][ks] = *reinterpret_cast<const bf16x8*>(     // fragment-major W1^T (kernels.h)
            wf1t + ((int64_t)(((f0 >> 4) + ft) * (HID / 32) + ks) * 64 + lane) * 8);
    }
    // keep every load above this point: the scheduler would otherwise interleave them
    // with the MFMAs behind per-load waits
    __builtin_amdgcn_sched_barrier(0);
    FC_STAMP(t, 1);
    f32x4 acc[DX_FT][2];
#pragma unroll
    for (int ft = 0; ft < DX_FT; ++ft)
#pragma unroll
      for (int bt = 0; bt < 2; ++bt) acc[ft][bt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < HID / 32; ++ks)
#pragma unroll
      for (int ft = 0; ft < DX_FT; ++ft)
#pragma unroll
        for (int bt = 0; bt < 2; ++bt)
          acc[ft][bt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hb[bt][ks], wa[ft][ks], acc[ft][bt], 0, 0, 0);
    FC_STAMP(t, 2);
    // D[b][f]: lane (g, i16) holds rows b = 4g + r of feature i16: a store covers 4 rows x 32 B
#pragma unroll
    for (int bt = 0; bt < 2; ++bt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = b0 + bt * 16 + 4 * g + r;
        if (row < B) {
#pragma unroll
          for (int ft = 0; ft < DX_FT; ++ft)
            st_ho<2>(&dpool[(int64_t)row * FEAT + f0 + ft * 16 + i16], to_bf16(acc[ft][bt][r]));
        }
      }
    FC_STAMP(t, 3);
    return;
  }

  // ---- head slab reduction: HR_BLOCKS workgroups x 64 slab columns x 4 slab groups ----
  // (the fp32 kernels' copy is head_slab_reduce in cnn_f32_common.h)
  {
    __shared__ float rs[4][64];
    __shared__ double rd[4][64];
    const int e = (bid - DW_TILES - nd) * 64 + (tid & 63), grp = tid >> 6;
    const int ec = min(e, HEAD_SLAB - 1);
    float s = 0.f;
    double sd = 0.0;
    for (int j0 = grp; j0 < head_blocks; j0 += 4 * 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        v[u] = head_slab[(int64_t)min(j0 + 4 * u, head_blocks - 1) * HEAD_SLAB + ec];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float x = (j0 + 4 * u < head_blocks) ? v[u] : 0.f;
        s += x;
        sd += (double)x;
      }
    }
    rs[grp][tid & 63] = s;
    rd[grp][tid & 63] = sd;
    __syncthreads();
    if (tid < 64 && e < HEAD_SLAB) {
      s = ((rs[0][tid] + rs[1][tid]) + rs[2][tid]) + rs[3][tid];
      sd = ((rd[0][tid] + rd[1][tid]) + rd[2][tid]) + rd[3][tid];
      if (e < NCLS * HID) gwf2[e] = s;
      else if (e < NCLS * HID + NCLS) gbf2[e - NCLS * HID] = s;
      else if (e < NCLS * HID + NCLS + HID) gbf1[e - NCLS * HID - NCLS] = s;
      else if (e == HEAD_SLAB - 2) { metrics[0] += sd; metrics[2] += (double)B; }
      else metrics[1] += sd;
    }
  }
}

}  // namespace

void launch_fc1_bwd(const __bf16* dh, const __bf16* dht, int ldt, const __bf16* pool,
                    const __bf16* wf1t, int B, float* gwf1, __bf16* dpool, const float* head_slab,
                    int head_blocks, float* gwf2, float* gbf2, float* gbf1, double* metrics,
                    const FcUpdate& fcu, hipStream_t st) {
  const int nd = (ldt / 32) * DX_TILES;
  const int nblk = DW_TILES + nd + HR_BLOCKS, off = 0;
  fc1_bwd_kernel<<<nblk, 256, 0, st>>>(dh, dht, ldt, pool, wf1t, B, gwf1, dpool, head_slab,
                                       head_blocks, gwf2, gbf2, gbf1, metrics, off, fcu);
}

PDM_STAMP_READER(fc1_bwd)
