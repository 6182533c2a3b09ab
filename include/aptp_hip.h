/*
 * aptp_hip.h — C ABI of libaptp_hip.so: the MI355X (gfx950) kernels behind APTP's masked-U-Net denoising path.
 *
 * The reference (rezashkv/diffusion_pruning) is pure Python and has no FFI boundary of its own; every entry point
 * below replaces a *call site into torch/diffusers* inside the reference's gated blocks.  Citations are
 * file:line relative to the reference tree.
 *
 * Conventions
 *   - All pointers are DEVICE pointers owned by the caller (PyTorch allocates everything, including workspaces).
 *   - Activations are bf16, channels-last: a conv input is [B, H, W, C] with a row (pixel) stride `ld*` in
 *     ELEMENTS, so strided channel-slices of wider buffers can be read/written in place (no torch.cat copies).
 *     A linear layer is the KH=KW=1 case with H = tokens per sample, W = 1.
 *   - Weights are pre-packed bf16 [N][KH*KW][Cin_pad] (K-contiguous), Cin_pad = ceil(Cin/64)*64, zero padded.
 *   - Epilogue vectors (bias, gates, corrections, depth) are fp32.
 *   - Every launch is asynchronous on `stream`; no hidden sync, no global state => hipGraph-capturable.
 *   - Return 0 on success, a negative APTP_E* code otherwise; aptp_last_error() gives a thread-local message.
 */
#ifndef APTP_HIP_H
#define APTP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* aptp_stream_t; /* hipStream_t */

enum {
  APTP_OK = 0,
  APTP_EINVAL = -1,   /* bad shape / alignment / null pointer */
  APTP_ELAUNCH = -2,  /* hipLaunch failed */
  APTP_EWORKSPACE = -3
};

/* APTP_ACT_GELU: exact (erf) GELU of the biased value, the hidden_act "gelu" of CLIP's text encoder (transformers CLIPMLP:
 * fc1 -> GELU -> fc2).  APTP_ACT_QUICK_GELU: v * sigmoid(1.702 v) of the biased value, the hidden_act "quick_gelu" of OpenAI's
 * CLIP checkpoints (transformers QuickGELUActivation; the vision tower CMMD embeds with, cmmd-pytorch/embedding.py:38).  Its value
 * is 5: 4 is reserved and, like any other value, refused by aptp_conv_gemm with APTP_EINVAL. */
enum { APTP_ACT_NONE = 0, APTP_ACT_SILU = 1, APTP_ACT_GEGLU = 2, APTP_ACT_GELU = 3, APTP_ACT_QUICK_GELU = 5 };

/*
 * Implicit-GEMM convolution / linear:  y[m, n] = epilogue( sum_{tap,c} x[pix(m,tap), c] * w[n, tap, c] )
 *   m = (b, oy, ox) over B*Hout*Wout,  pix = (b, (oy*stride - pad + ky) >> u, (ox*stride - pad + kx) >> u)
 *   ups = 0: u = 0;  ups = 1: u = 1 (nearest x2 upsample folded into the gather);  ups = 2: u = 1 and odd coordinates read
 *   zero (zero-insertion x2 = the data-gradient of a stride-2 convolution, with flipped/transposed packed weights)
 * Replaces: F.conv2d in ResnetBlock2D*.conv1/conv2/conv_shortcut (pdm/models/unet/blocks.py:331,362,364-367,
 * 537,568,570-573), Downsample2D/Upsample2D convs (inherited diffusers; nearest-x2 folded via `ups`),
 * conv_in/conv_out (pdm/models/unet/unet_2d_conditional.py:1614,1721), and every F.linear of the transformer
 * path: to_q/to_k/to_v/to_out (blocks.py:228-240,266-268), GEGLU proj (blocks.py:43), ff.net[2], proj_in/proj_out
 * (blocks.py:1239-1243,1301-1305), time_emb_proj (blocks.py:336-340), time_embedding
 * (unet_2d_conditional.py:1519).
 * Epilogue, in this order (each optional):
 *   v += bias[n]; v += rowbias[b, n]                      (conv bias; + time_emb_proj(SiLU(temb)), blocks.py:342-343)
 *   v *= colgate[b % gate_B, n / gate_group]              (WidthGate, gates.py:15-21; blocks.py:345-348, 250-255)
 *   act: SiLU, or GEGLU on (h,g) column pairs: h * gelu_erf(g)   (blocks.py:41-50; gate applied to both halves),
 *        or GELU: gelu_erf(v), or QUICK_GELU: v * sigmoid(1.702 v)    (CLIPMLP.fc1 + activation_fn; split-K: applied by
 *        whichever launch sums the K-slices)
 *   v += corr[(b % corr_B), border_class(oy,ox), n]       (gated-vs-pruned GroupNorm-beta term)
 *   v += residual[m, n]                                   (blocks.py:369, 799, 818, 849, 1308)
 *   v = (1-d[b % depth_B]) * depth_in[m, n] + d * v       (DepthGate, gates.py:36-42; blocks.py:577-582,1345-1348)
 */
typedef struct {
  const void* x;        /* bf16 [B, Hin, Win, >=Cin], row stride ldx */
  int64_t ldx;
  int32_t B, Hin, Win, Cin;
  int32_t Hout, Wout;
  int32_t KH, KW, stride, pad, ups;
  const void* w;        /* bf16 packed [N][KH*KW][Cin_pad] */
  int32_t N;            /* GEMM N (for GEGLU: 2*hidden, packed in [16 h | 16 g] column blocks) */
  int32_t cin_pad;      /* ceil(Cin/64)*64 */
  const float* bias;    /* [N] or NULL */
  const float* rowbias; /* [B, ld_rowbias] or NULL */
  int32_t ld_rowbias;
  const float* colgate; /* [gate_B, Nlogical/gate_group] or NULL */
  int32_t gate_group, gate_B;
  int32_t act;          /* APTP_ACT_* */
  const float* corr;    /* [corr_B, 9, N] or NULL; class = 3*rowclass + colclass (0 first / 1 interior / 2 last row or column), class 4 = interior */
  int32_t corr_B;
  const void* residual; /* bf16 [M, ldres] or NULL */
  int64_t ldres;
  const float* depth;   /* [depth_B] or NULL */
  int32_t depth_B;
  const void* depth_in; /* bf16 [M, lddin] */
  int64_t lddin;
  void* y;              /* bf16 (or fp32 if out_f32) [M, ldy]; GEGLU writes N/2 columns */
  int64_t ldy;
  int32_t out_f32;
  int32_t split_k;      /* >=1; >1 needs workspace of aptp_conv_gemm_workspace_bytes() */
  void* workspace;
  int32_t tile;         /* 0 = auto; otherwise APTP_TILE_* (testing / tuning) */
  int32_t order;        /* workgroup -> tile order over the 8 XCDs: 0 = auto (partition the larger operand), 1 = legacy
                         * (N-tile fastest), 2 = weight-major, 3 = activation-major (testing / tuning) */
  /* LayerNorm folded into the neighbouring GEMMs (nn.LayerNorm norm1/norm2/norm3 of BasicTransformerBlock,
   * blocks.py:782,808-810,821; inference path).  The GEMM that PRODUCES the normalised tensor (proj_in, to_out with its
   * residual) also emits, per output row, fp32 (sum, sumsq) partials of the bf16 values it stores, one per (N-tile, wave
   * column): rowstat_out [rowstat_slots / 2, M, 2, 2] (two slots per 16-byte element; the slot count is always even),
   * rowstat_slots = aptp_conv_gemm_rowstat_slots(); needs split_k == 1 or tile_counters, a bf16
   * non-GEGLU output.  The GEMM that CONSUMES LayerNorm(x) reads x itself with gamma folded into its packed weights
   * (w' = w * gamma) and finishes the normalisation in its epilogue, before bias:
   *     v = rstd[m] * (acc[m, n] - mean[m] * ln_colsum[n]),   mean/rstd from ln_stats [ln_slots / 2, M, 2, 2] over ln_C channels,
   * ln_colsum[n] = sum_k bf16(w'[n, k]) (fp32), and the caller adds sum_k beta[k] w[n, k] to bias[n]. */
  float* rowstat_out;
  int32_t rowstat_slots;
  const float* ln_stats;
  int32_t ln_slots;
  const float* ln_colsum;
  float ln_eps;
  int32_t ln_C;
  /* GroupNorm statistics emitted by the producer (F.group_norm of ResnetBlock2D.norm1 / norm2, Transformer2DModel.norm,
   * conv_norm_out: blocks.py:296-301,350-359,1227; unet_2d_conditional.py:1718): per channel, fp32 (sum, sumsq) of the
   * bf16 values stored for each block of R = aptp_conv_gemm_colstat_rows() consecutive output rows, colstat_out
   * [ceil(M/R) rounded up to whole tiles, colstat_ld, 2].  Needs Hout*Wout % R == 0 (a block never straddles samples),
   * a bf16 non-GEGLU output with 16-byte aligned rows, split_k == 1 or the in-kernel reduction.  aptp_groupnorm consumes
   * them through AptpGroupNormParams.colstats and skips its own statistics pass. */
  float* colstat_out;
  int32_t colstat_ld;
  int32_t* tile_counters; /* optional, split_k > 1: >= aptp_conv_gemm_tiles() int32 words, ZERO on entry and left zero: the
                           * K-slices are then combined inside the launch by the last-arriving workgroup of each output tile
                           * (one agent-scope release / acquire per tile, slabs re-read in slice order: deterministic) and no
                           * reduce kernel is launched; words may be shared by launches of one stream */
  /* optional second operand: one more K-segment after the KH*KW filter taps, read AT the output pixel (a 1x1 "tap") over
   * the Cin2 channels of x2 [B, Hout, Wout, >=Cin2] (row stride ldx2); the packed weights are then
   * [N][KH*KW*cin_pad + cin2_pad].  Fuses ResnetBlock2D.conv_shortcut (blocks.py:364-367,570-573) into conv2:
   * conv2(h) + conv_shortcut(x) is one GEMM with K = 9*C_mid + C_in, the shortcut never round-trips through memory and
   * its bias is added to conv2's.  Needs stride 1, no upsampling, Hout == Hin, Wout == Win. */
  const void* x2;
  int64_t ldx2;
  int32_t Cin2, cin2_pad;
  /* optional: [prefetch, prefetch + prefetch_bytes) = an operand of the NEXT launch (its packed weights).  The workgroups
   * touch it at kernel entry (one dword per 64-byte line, results discarded), each XCD its eighth of the buffer -- the rows
   * the weight-major order of the next launch gives that XCD -- so that the weights are in the right L2 when the next launch
   * starts: every weight of the U-Net is read once per forward and would otherwise be fetched cold.  Pays for buffers that
   * fit the L2s (<= ~12 MB); 4-byte aligned. */
  const void* prefetch;
  int64_t prefetch_bytes;
  int32_t epilogue;     /* 0 = auto (coalesced 16-byte stores through an LDS transpose when y / residual / depth_in rows are
                         * 16-byte aligned), 1 = force the accumulator-layout epilogue (testing / tuning), 2 = keep a plain linear layer on the
                         * general implicit-GEMM kernel instead of the lean one of csrc/lin_gemm.hip (testing: the two must agree).  1 and 2 also
                         * keep a 3x3 convolution on the general kernel instead of the lean one of csrc/conv_lean.hip (bit-identical outputs) */
  /* optional, small maps (Hout*Wout <= 256), split_k > 1 without tile_counters: the reduce launch of the split also applies
   * the GroupNorm(+SiLU) that follows this convolution (ResnetBlock2D: conv1 + time_emb_proj -> norm2 -> SiLU,
   * blocks.py:331-359): one workgroup per (sample, group) sums the K-slices of its Hout*Wout x (gn_C / gn_groups) columns,
   * adds bias / rowbias, rounds to bf16 (the value the separate launches would have stored), takes the group's statistics,
   * and writes y = act(gamma * (h - mean) * rstd + beta) -- y is then the NORMALISED tensor; the convolution output itself
   * is never stored.  Needs act == NONE and no colgate / corr / residual / depth / statistics outputs, gn_C % 8 == 0,
   * (gn_C / gn_groups) % 4 == 0; columns >= gn_C of y are written as zeros. */
  const float* gn_gamma;  /* [gn_C] or NULL (= feature off) */
  const float* gn_beta;
  int32_t gn_groups, gn_C, gn_silu;
  float gn_eps;
  /* fp32 PARITY instantiation (never benchmarked): x, w (packed fp32 [N][KH*KW][Cin_pad]), x2, residual, depth_in and y are fp32
   * tensors (out_f32 must be 1; row strides in elements as always), the contraction runs on exact-fp32 MFMAs
   * (v_mfma_f32_16x16x4_f32) through the SAME gather / tap walk / zero padding / split-K / epilogue code as the bf16
   * register-staged kernel (tiles 1..6 only).  Pins addressing and epilogue order on the GPU against the fp32 oracle at 1e-5
   * per op; the reference computes in fp32 (configs/pruning/sd-2-1_cc3m.yaml:79). */
  int32_t io_f32;
  /* round 4, optional, together with colstat_out: GroupNorm statistics the consumer can use WITHOUT a finalise launch.  Every
   * wave that emits column statistics also adds, per channel unit of `ustat_unit` consecutive output channels it touches, the
   * (sum, sum of squares) of its stored values to ustat_out[rep][sample][unit][2] -- int64 fixed point (sum * 2^20, squares *
   * 2^12), 64-bit integer atomics: the totals do not depend on the order of arrival (deterministic), `ustat_nrep` (a power of
   * two) replicas selected by the workgroup index spread the contention.  The buffer must be ZERO on entry
   * (nrep * B * ustat_units * 2 words, ustat_units = ceil(N_out / ustat_unit)); nobody resets it. */
  void* ustat_out;
  int32_t ustat_unit, ustat_units, ustat_nrep;
  /* extra zero rows and columns AFTER the input's last row and column (>= 0): the output extent is
   * Hout = (Hin' + 2 * pad + pad_end - KH) / stride + 1 (and the same for W).  diffusers Downsample2D with padding 0
   * (the VAE encoder: F.pad(x, (0, 1, 0, 1)) followed by a stride-2, pad-0 3x3 convolution) is pad = 0, pad_end = 1.
   * The gathers already read zeros past the input, so the general, LDS-DMA, stream-K and fp32 parity kernels take it
   * unchanged; pad_end > 0 refuses corr, x2, ups and the halo tiles, and never takes the lean linear / 3x3 kernels. */
  int32_t pad_end;
} AptpConvGemmParams;

/* The documented numbering.  Each id's geometry, kernel family and lean instantiations are its row of csrc/conv_gemm_tiles.h,
 * which fails the build when a row's position and the value here disagree. */
enum { APTP_TILE_AUTO = 0, APTP_TILE_128x128 = 1, APTP_TILE_128x160 = 2, APTP_TILE_64x128 = 3, APTP_TILE_64x160 = 4,
       APTP_TILE_128x64 = 5, APTP_TILE_64x64 = 6,
       /* same tiles, operands copied global->LDS by LDS-DMA instead of through registers */
       APTP_TILE_DMA_128x128 = 7, APTP_TILE_DMA_128x160 = 8, APTP_TILE_DMA_64x128 = 9, APTP_TILE_DMA_64x160 = 10,
       APTP_TILE_DMA_128x64 = 11, APTP_TILE_DMA_64x64 = 12,
       /* LDS-DMA with a 3-deep ring (DMA two K-steps ahead, counted vmcnt + raw barrier) */
       APTP_TILE_DMA3_128x128 = 13, APTP_TILE_DMA3_128x160 = 14, APTP_TILE_DMA3_64x128 = 15, APTP_TILE_DMA3_64x160 = 16,
       APTP_TILE_DMA3_128x64 = 17, APTP_TILE_DMA3_64x64 = 18,
       /* LDS-DMA, 8-wave (512-thread) workgroups: one weight tile shared by twice the rows */
       APTP_TILE_DMA8_128x160 = 19, APTP_TILE_DMA8_256x160 = 20, APTP_TILE_DMA8_128x128 = 21, APTP_TILE_DMA8_256x128 = 22,
       /* LDS-DMA, 4 waves, 4-stage ring (three operand tiles in flight) */
       APTP_TILE_DMA4_64x160 = 23, APTP_TILE_DMA4_64x128 = 24, APTP_TILE_DMA4_64x64 = 25, APTP_TILE_DMA4_128x64 = 26,
       APTP_TILE_DMA4_128x128 = 27,
       /* LDS-DMA, 8 waves, 3- or 4-stage ring */
       APTP_TILE_DMA8R3_128x160 = 28, APTP_TILE_DMA8R4_128x160 = 29, APTP_TILE_DMA8R3_128x128 = 30,
       APTP_TILE_DMA8R4_128x128 = 31, APTP_TILE_DMA8R3_256x128 = 32,
       /* LDS-DMA, 8 waves in two groups that alternate load and MFMA slots (ping-pong), 3- or 4-stage ring */
       APTP_TILE_PP3_128x160 = 33, APTP_TILE_PP4_128x160 = 34, APTP_TILE_PP3_128x128 = 35, APTP_TILE_PP4_128x128 = 36,
       APTP_TILE_PP4_64x160 = 37, APTP_TILE_PP4_64x128 = 38, APTP_TILE_PP5_64x160 = 39, APTP_TILE_PP4_128x64 = 40,
       APTP_TILE_PP3_256x128 = 41, APTP_TILE_PP3_128x256 = 42,
       /* 3x3 / stride-1 / pad-1 only, image width 16 / 32 / 64: the input halo of 128 output pixels (whole image rows) is
        * kept in LDS across the nine taps, weights stream through a 4-stage ring (8 waves) */
       APTP_TILE_HALO_128x160 = 43, APTP_TILE_HALO_128x128 = 44,
       /* LDS-DMA, 4 waves, 6- or 8-stage ring (96-144 KB of LDS, one workgroup per CU): launches with few workgroups and a
        * long K whose time is K-steps x operand latency / tiles in flight */
       APTP_TILE_DMA6_64x64 = 45, APTP_TILE_DMA8S_64x64 = 46, APTP_TILE_DMA6_64x128 = 47, APTP_TILE_DMA6_128x64 = 48,
       /* LDS-DMA ring with TWO 64-wide K-tiles per barrier (an effective K-step of 128), 4- or 6-stage ring; 4 waves, the
        * last two 8 waves */
       APTP_TILE_KU2S4_64x64 = 49, APTP_TILE_KU2S6_64x64 = 50, APTP_TILE_KU2S4_64x128 = 51, APTP_TILE_KU2S6_64x128 = 52,
       APTP_TILE_KU2S4_128x64 = 53, APTP_TILE_KU2S4_128x128 = 54, APTP_TILE_KU2S4_64x160 = 55, APTP_TILE_KU2S4_128x160 = 56,
       APTP_TILE_KU2S4_128x128W8 = 57,
       /* LDS-DMA ring, 8 waves as TWO copies of a 2 x 2 wave grid: copy 0 / 1 multiplies the first / second 32-wide half
        * of every K-tile (intra-workgroup split-K, summed through LDS before the epilogue); 3- or 4-stage ring */
       APTP_TILE_KS2S3_64x64 = 58, APTP_TILE_KS2S4_64x64 = 59, APTP_TILE_KS2S3_64x128 = 60, APTP_TILE_KS2S4_64x128 = 61,
       APTP_TILE_KS2S3_128x64 = 62, APTP_TILE_KS2S3_128x128 = 63,
       /* persistent stream-K macro-tiles (conv_gemm_sk.hip): one 8-wave workgroup per CU walks an equal share of the
        * launch's (tile, K-step) units; split_k > 1 = K split on (needs workspace + tile_counters: partial tiles are
        * combined in-kernel by the last arriver), split_k == 1 = whole tiles only.  Two wave groups alternate an LDS /
        * load slot and a register-only MFMA slot per 32-deep K half; 3-stage LDS-DMA ring filled in half-tiles */
       APTP_TILE_SK_256x160 = 64, APTP_TILE_SK_256x128 = 65, APTP_TILE_SK_128x256 = 66,
       /* the same with a phase's fragment reads in its own load slot (beside the OTHER group's MFMAs) instead of one phase
        * ahead beside the wave's own MFMAs: one register set, shorter DMA lead (tuner candidates) */
       APTP_TILE_SKL_256x160 = 67, APTP_TILE_SKL_256x128 = 68, APTP_TILE_SKL_128x256 = 69,
       /* round 4: the same persistent stream-K kernels on 128-row tiles -- the tile sizes the batch-4 launches fill the chip with
        * (128 tiles of 128 x 160 at level 64 = one two-way split per tile, like the ping-pong tile's own split-K), with the
        * macro-tile kernel's per-lane offset tables and two-slot schedule instead of the per-step tap logic */
       APTP_TILE_SK_128x160 = 70, APTP_TILE_SKL_128x160 = 71, APTP_TILE_SK_128x128 = 72, APTP_TILE_SKL_128x128 = 73 };

int aptp_conv_gemm(const AptpConvGemmParams* p, aptp_stream_t stream);
int64_t aptp_conv_gemm_workspace_bytes(const AptpConvGemmParams* p);
/* rows per statistics block of colstat_out for the tile the launch will use */
int aptp_conv_gemm_colstat_rows(const AptpConvGemmParams* p);
/* output tiles of the launch (size of tile_counters) */
int aptp_conv_gemm_tiles(const AptpConvGemmParams* p);
/* number of row-statistics slots a launch of this problem writes per row (N-tiles x wave columns of the tile it will use) */
int aptp_conv_gemm_rowstat_slots(const AptpConvGemmParams* p);
/* heuristic split-K the library would choose for this problem (host helper, no launch) */
int aptp_conv_gemm_suggest_split_k(const AptpConvGemmParams* p);

/*
 * GroupNorm (+ optional SiLU) over channels-last bf16:  y = act((x - mean_g) * rstd_g * gamma + beta)
 * Replaces F.group_norm + F.silu of ResnetBlock2D.norm1/norm2 + nonlinearity (blocks.py:296-301,350-359),
 * Transformer2DModel.norm (blocks.py:1227, eps 1e-6, no SiLU) and conv_norm_out + conv_act
 * (unet_2d_conditional.py:1718-1720).  `groups` groups of C/groups consecutive channels; statistics over
 * (C/groups)*HW elements per (sample, group), biased variance, fp32 accumulation.
 * C need not be a multiple of 8 (compacted channel counts such as 17 groups x 10): rows are processed in 8-channel
 * octets, ld >= roundup8(C), and channels [C, roundup8(C)) of y are written as exact zeros.
 * workspace: aptp_groupnorm_workspace_bytes() = fp32 [B, nchunk, groups, 2] (sum, sumsq) partials, nchunk =
 * aptp_groupnorm_nchunk(HW), followed by the finalised [B, groups, 2] (mean, rstd).
 */
/* one channel segment of producer-emitted statistics (AptpConvGemmParams.colstat_out) */
typedef struct {
  const float* stats;       /* [B*HW/rows_per_block (+ padding blocks), ld, 2] or NULL */
  int32_t ld, rows_per_block, C;
  /* round 4, optional: the same producer also left per-(sample, channel UNIT) sums (AptpConvGemmParams.ustat_out): int64
   * fixed point [nrep][B][units][2] (sum * 2^20, sum of squares * 2^12), `unit` channels per unit.  When every segment has
   * them, C of every segment and C / groups are multiples of `unit`, the apply pass finishes mean / rstd itself and NO
   * finalise launch runs (one launch per GroupNorm). */
  const void* ustats;
  int32_t unit, units, nrep;
} AptpGroupNormColStats;

typedef struct {
  const void* x; int64_t ldx;   /* bf16 [B*HW, >=C] */
  void* y; int64_t ldy;         /* bf16 [B*HW, >=C] */
  int32_t B, HW, C, groups;
  const float* gamma; const float* beta; /* [C] */
  float eps;
  int32_t silu;
  void* workspace;
  /* 0 = auto; 1 = three launches (stats, finalise, apply), which fill the workspace partials aptp_groupnorm_bwd consumes;
   * 2 = one launch, each workgroup owning whole groups of one sample (small maps);
   * 3 = two launches: at most 16 coarse statistics chunks, folded by every apply workgroup (no finalise launch);
   * 4 = auto WITH those partials: the small maps still take one launch (the owning workgroup writes its groups' sums into
   *     chunk 0 and zeros into the other chunks), everything else the three-launch form. */
  int32_t variant;
  /* optional, three-launch form only: >= B int32 words, ZERO on entry and left zero.  The last statistics workgroup of
   * each sample then folds the partials itself (write-through partial stores, one agent-scope acquire) and the
   * finalise launch is skipped: two launches instead of three. */
  int32_t* counters;
  /* optional: the statistics were emitted by the GEMM(s) that produced x -- one segment, or two for a skip-concat
   * (segment 0 = channels [0, C0), segment 1 = [C0, C)).  The statistics pass over x is skipped: a (groups x B)-workgroup
   * finalise from the partials, then the apply pass (two launches, x read once). */
  AptpGroupNormColStats colstats[2];
  /* fp32 PARITY path (csrc/parity_f32.hip; never benchmarked): x and y are fp32, three plain launches with the product's
   * statistics layout and variance formula; no producer statistics, no fused finalize */
  int32_t io_f32;
} AptpGroupNormParams;

int aptp_groupnorm(const AptpGroupNormParams* p, aptp_stream_t stream);
int aptp_groupnorm_nchunk(int HW);
int aptp_rows_nchunk(int rows);   /* row chunks of the kernels without a batch dimension (aptp_layernorm_pgrad, aptp_colsum with batch <= 1) */
int64_t aptp_groupnorm_workspace_bytes(const AptpGroupNormParams* p);

/*
 * LayerNorm over the last dim of bf16 [rows, C]: replaces nn.LayerNorm norm1/norm2/norm3 of
 * BasicTransformerBlock (blocks.py:782,808-810,821); eps 1e-5, affine, two-pass fp32 statistics.
 */
typedef struct {
  const void* x; int64_t ldx;
  void* y; int64_t ldy;
  int32_t rows, C;
  const float* gamma; const float* beta;
  float eps;
  int32_t io_f32;   /* fp32 PARITY path: x and y are fp32 (csrc/parity_f32.hip) */
} AptpLayerNormParams;

int aptp_layernorm(const AptpLayerNormParams* p, aptp_stream_t stream);

/*
 * Scaled-dot-product attention, head_dim 64, no mask, no dropout: o = softmax(q k^T * scale) v per (batch, head).
 * Replaces F.scaled_dot_product_attention in HeadGatedAttnProcessor2 (blocks.py:258-260).
 * q/k/v/o are bf16 with layout [B, L, heads, 64] expressed through strides (elements): element (b, l, h, d) at
 * ptr + b*stride_b + l*stride_l + h*64 + d, so fused QKV / KV GEMM outputs are consumed in place.
 * APTP_EINVAL and nothing launched for: null pointers, extents < 1, strides that are not multiples of 8 elements (o: 4),
 * misaligned pointers, a row stride below heads*64, and (bf16 path) scale <= 0 or NaN.
 */
typedef struct {
  const void* q; int64_t q_stride_b, q_stride_l;
  const void* k; int64_t k_stride_b, k_stride_l;
  const void* v; int64_t v_stride_b, v_stride_l;
  void* o; int64_t o_stride_b, o_stride_l;
  int32_t B, heads, Lq, Lk;
  float scale;  /* > 0: the kernels take the running maximum over the raw scores */
  float* lse;  /* optional fp32 [B, heads, Lq]: log2-domain log-sum-exp of the scaled scores, consumed by aptp_attention_bwd */
  int32_t variant; /* 0 = auto; 1 = run the two key-range wave groups of the 8-wave kernel one phase apart (double-buffered
                    * K/V; measured slower than the lock-step form, kept for testing / A-B timing); 2 = force four key-range
                    * groups (16 waves); 3 = force two lock-step groups with single-buffered K/V (two barriers per key tile);
                    * 4 = force two lock-step groups with double-buffered K/V (one barrier per key tile; auto from 32 key
                    * tiles); 5 = force the 4-wave kernel (one group); 6 = the software-pipelined two-group kernel (round 4:
                    * scores of key tile i+1 next to the softmax of tile i, V read transposed in hardware), which is also
                    * what auto takes whenever Lq % 128 == 0, Lk % 128 == 0, Lk >= 256 -- bit-identical to variant 4.
                    * An explicit variant overrides the occupancy rule that otherwise chooses between one and two groups */
  int32_t io_f32;  /* fp32 PARITY path: q, k, v, o are fp32 (strides in elements), no lse (csrc/parity_f32.hip) */
} AptpAttentionParams;

int aptp_attention(const AptpAttentionParams* p, aptp_stream_t stream);

/*
 * The two non-GEMM ends of UNet2DConditionModel.forward (unet_2d_conditional.py:1497-1519 time embedding input,
 * :1614 conv_in input layout, :1721-1726 output): one launch each instead of ~10 elementwise kernels.
 *   prologue: sample [B, C, H, W] (fp32, or bf16 when sample_bf16) -> x bf16 [B, H, W, cin_pad] (padding channels zero);
 *             t_emb[b] = [cos(timesteps[b] * freqs[k]) | sin(timesteps[b] * freqs[k])], k < half, as bf16 [B, 2*half]
 *             (diffusers get_timestep_embedding with flip_sin_to_cos = True).
 *   epilogue: y fp32 [B, H, W, ldy] (conv_out) -> out [B, C, H, W] (fp32, or bf16 when out_bf16).
 */
typedef struct {
  const void* sample; int32_t sample_bf16;
  void* x;
  int32_t B, C, H, W, cin_pad;
  const float* timesteps;   /* fp32 [B] */
  const float* freqs;       /* fp32 [half] */
  int32_t half;
  void* t_emb;              /* bf16 [B, 2*half] */
} AptpUnetPrologueParams;

typedef struct {
  const float* y; int64_t ldy;
  void* out; int32_t out_bf16;
  int32_t B, C, H, W;
} AptpUnetEpilogueParams;

int aptp_unet_prologue(const AptpUnetPrologueParams* p, aptp_stream_t stream);
int aptp_unet_epilogue(const AptpUnetEpilogueParams* p, aptp_stream_t stream);

/*
 * Single-head attention of width 512, no mask: o = softmax(q k^T * scale) v per sample, fp32 softmax statistics.
 * Replaces the mid-block self-attention of AutoencoderKL's decoder (diffusers Attention, heads = 1, dim_head = 512,
 * upcast_softmax; default scale 512^-0.5).  q/k/v/o are bf16 [B, L, 512] expressed through strides (elements): element
 * (b, l, c) at ptr + b*stride_b + l*stride_l + c, so a fused q|k|v GEMM output is consumed in place.  Row and batch strides
 * are multiples of 8 elements, pointers 16-byte aligned; any Lq, Lk >= 1.
 */
typedef struct {
  const void* q; int64_t q_stride_b, q_stride_l;
  const void* k; int64_t k_stride_b, k_stride_l;
  const void* v; int64_t v_stride_b, v_stride_l;
  void* o; int64_t o_stride_b, o_stride_l;
  int32_t B, Lq, Lk;
  float scale;       /* > 0 */
  int32_t io_f32;    /* fp32 PARITY path: q, k, v, o are fp32 (strides multiples of 4), exact-fp32 arithmetic; never benchmarked */
} AptpAttentionWideParams;

int aptp_attention_wide(const AptpAttentionWideParams* p, aptp_stream_t stream);

/*
 * Image epilogue of the VAE decoder (diffusers VaeImageProcessor.postprocess with do_denormalize, then numpy_to_pil):
 * y fp32 [B, H, W, ldy] (conv_out, 3 real channels) -> v = clamp(y / 2 + 0.5, 0, 1), written either as fp32 [B, 3, H, W]
 * (out_u8 = 0) or as uint8 [B, H, W, 3] = round_half_even(v * 255) (out_u8 = 1).
 */
typedef struct {
  const float* y; int64_t ldy;
  void* out; int32_t out_u8;
  int32_t B, H, W;
} AptpImageOutParams;

int aptp_image_out(const AptpImageOutParams* p, aptp_stream_t stream);

/*
 * Image prologue of the VAE encoder: pixel_values NCHW [B, 3, H, W] (fp32 or bf16, in [-1, 1]) -> the 3x3 / pad-1 im2col of
 * every pixel, out [B, H, W, 32] tap-major: element (ky * 3 + kx) * 3 + c = x[b, c, y + ky - 1, x + kx - 1] (zero outside the
 * image), elements 27..31 zero.  encoder.conv_in (3 -> 128, 3x3) then runs as a 1x1 contraction over 32 channels with the
 * weight repacked as w'[o][(ky * 3 + kx) * 3 + c] = w[o][c][ky][kx].  out is bf16, or fp32 (out_f32: the parity path).
 */
typedef struct {
  const void* x; int32_t x_bf16;
  void* out; int32_t out_f32;
  int32_t B, C, H, W;   /* C must be 3 */
} AptpImageInParams;

int aptp_image_in(const AptpImageInParams* p, aptp_stream_t stream);

/*
 * The end of AutoencoderKL.encode: quant_conv (8 x 8 matrix + bias, fp32) on conv_out's fp32 [B, H, W, ldy] (8 real
 * channels), written NCHW as diffusers' moments [B, 8, H, W] fp32 (DiagonalGaussianDistribution.parameters), and
 * optionally the sample: given eps fp32 NCHW [B, 4, H, W],
 *     latents = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * eps)      (mean = moments[:, :4], logvar = moments[:, 4:])
 * as fp32 or bf16 NCHW [B, 4, H, W].  Every operation is one explicitly rounded fp32 operation (no FMA contraction), in the
 * order written, the quant_conv sum in input-channel order; no atomics (deterministic).  scale == 1 gives the plain
 * sample; the scale multiply is last, so scale * sample(scale 1) in fp32 is bit-identical to the scaled launch.
 */
typedef struct {
  const float* y; int64_t ldy;     /* fp32 [B, H, W, ldy], ldy >= 8 */
  const float* wq;                 /* fp32 [8][8] (out, in) */
  const float* bq;                 /* fp32 [8] */
  float* moments;                  /* fp32 [B, 8, H, W] or NULL */
  const float* eps;                /* fp32 [B, 4, H, W] or NULL (no sample) */
  void* latents; int32_t latents_bf16;
  float scale;
  int32_t B, H, W;
} AptpLatentDistParams;

int aptp_latent_dist(const AptpLatentDistParams* p, aptp_stream_t stream);

/*
 * Causal self-attention of short sequences, head_dim 64: o = softmax(q k^T * scale + causal) v per (batch, head), where key
 * j > query i gets weight exactly 0 (it never reaches the row maximum and adds 0 to the row sum); no padding mask.
 * Replaces the self-attention of CLIP's text encoder (transformers 4.34 CLIPAttention with the causal mask built by
 * CLIPTextTransformer; SD-2.1: 16 heads, L = 77, scale 64^-0.5), called through text_encoder(input_ids) at
 * pdm/training/trainer.py:1126,1443,1713 and encode_prompt, pdm/pipelines/pruning_pipelines.py:735-744.
 * Same strided layout as aptp_attention: element (b, l, h, d) at ptr + b*stride_b + l*stride_l + h*64 + d (a fused q|k|v
 * linear output is read in place).  1 <= L <= 128 (else APTP_EINVAL); row strides >= heads*64; strides multiples of 8
 * elements (4 for io_f32), pointers 16-byte aligned.  bf16 MFMA contractions, fp32 softmax statistics.
 */
typedef struct {
  const void* q; int64_t q_stride_b, q_stride_l;
  const void* k; int64_t k_stride_b, k_stride_l;
  const void* v; int64_t v_stride_b, v_stride_l;
  void* o; int64_t o_stride_b, o_stride_l;
  int32_t B, heads, L;
  float scale;       /* > 0 */
  int32_t io_f32;    /* fp32 PARITY path: q, k, v, o are fp32, exact-fp32 arithmetic; never benchmarked */
} AptpAttentionCausalParams;

int aptp_attention_causal(const AptpAttentionCausalParams* p, aptp_stream_t stream);

/*
 * CLIP text embeddings (transformers CLIPTextEmbeddings: token_embedding(input_ids) + position_embedding(position_ids) with
 * position_ids = 0..L-1), the first step of text_encoder(input_ids) (pdm/training/trainer.py:1126,1713):
 *     out[b*L + l, c] = bf16(tok[ids[b, l], c] + pos[l, c])    (fp32 sum, one rounding; fp32 out when out_f32)
 * ids int64 [B, L] contiguous, tok fp32 [vocab, C], pos fp32 [pos_rows, C], both contiguous; C a multiple of 8; L <= pos_rows
 * (else APTP_EINVAL).  An id outside [0, vocab) is never used as an index: its row is written as NaN.
 */
typedef struct {
  const int64_t* ids;
  const float* tok;
  const float* pos;
  void* out; int64_t ldo;     /* [B*L, ldo], ldo >= C, a multiple of 8 */
  int32_t B, L, C, vocab;
  int32_t out_f32;
  int32_t pos_rows;           /* rows of pos (max_position_embeddings) */
} AptpTokenEmbedParams;

int aptp_token_embed(const AptpTokenEmbedParams* p, aptp_stream_t stream);

/*
 * Bidirectional self-attention with a relative-position bias and a key padding mask, head_dim 64 (transformers
 * MPNetSelfAttention with the position_bias of MPNetEncoder.compute_position_bias and the extended attention mask), the
 * self-attention of the router's prompt encoder (sentence-transformers/all-mpnet-base-v2, pdm/utils/data_utils.py:130-155):
 *     o[b, i, h] = softmax_j(q[b, i, h] . k[b, j, h] * scale + relbias[h, j - i + L - 1] + (key_mask[b, j] ? 0 : -inf)) v[b, j, h]
 * relbias fp32 [heads, 2L - 1] contiguous (the bias depends on j - i only); key_mask fp32 [B, L] contiguous, any 0 / non-zero
 * pattern (not only a prefix), or NULL for "all valid".  A masked key gets weight exactly 0 whenever the row has a valid key
 * (its K and V are not even read into the contraction).  Query rows at or past the sample's last valid key are padding and are
 * written as zeros (a sample whose mask is all zero: every row zero); other masked query rows get finite values nobody reads.
 * Same strided layout as aptp_attention_causal: element (b, l, h, d) at ptr + b*stride_b + l*stride_l + h*64 + d (a fused
 * q|k|v linear output is read in place).  1 <= L <= 512 (else APTP_EINVAL); row strides >= heads*64; strides multiples of 8
 * elements (4 for io_f32), pointers 16-byte aligned.  bf16 MFMA contractions, fp32 softmax statistics.
 */
typedef struct {
  const void* q; int64_t q_stride_b, q_stride_l;
  const void* k; int64_t k_stride_b, k_stride_l;
  const void* v; int64_t v_stride_b, v_stride_l;
  void* o; int64_t o_stride_b, o_stride_l;
  const float* relbias;    /* fp32 [heads, 2L - 1] */
  const float* key_mask;   /* fp32 [B, L] or NULL */
  int32_t B, heads, L;
  float scale;       /* > 0 */
  int32_t io_f32;    /* fp32 PARITY path: q, k, v, o are fp32, exact-fp32 arithmetic; never benchmarked */
} AptpAttentionBiasParams;

int aptp_attention_bias(const AptpAttentionBiasParams* p, aptp_stream_t stream);

/*
 * MPNet embeddings (transformers MPNetEmbeddings in eval mode) in one launch, per token row (b, l):
 *     pos_id = (ids[b, l] != pad_id ? #{j <= l : ids[b, j] != pad_id} : 0) + pad_id        (create_position_ids_from_input_ids)
 *     out    = LayerNorm(word[ids[b, l]] + pos[pos_id]) * gamma + beta                      (fp32 sum, fp32 two-pass statistics)
 * rounded once to bf16 (fp32 out when out_f32).  ids int64 [B, L] contiguous; word fp32 [vocab, C], pos fp32 [pos_rows, C],
 * gamma / beta fp32 [C], all contiguous; C a multiple of 8, <= 2048; L + pad_id < pos_rows (else APTP_EINVAL).  An id outside
 * [0, vocab) is never used as an index: its row is written as NaN.
 */
typedef struct {
  const int64_t* ids;
  const float* word;
  const float* pos;
  const float* gamma;
  const float* beta;
  void* out; int64_t ldo;     /* [B*L, ldo], ldo >= C, a multiple of 8 */
  int32_t B, L, C, vocab;
  int32_t pos_rows;           /* rows of pos (max_position_embeddings) */
  int32_t pad_id;
  int32_t out_f32;
  float eps;
} AptpEmbedLnParams;

int aptp_embed_ln(const AptpEmbedLnParams* p, aptp_stream_t stream);

/*
 * Masked mean over the tokens (get_mpnet_embeddings, pdm/utils/data_utils.py:130-155; NOT L2-normalised):
 *     out[b, c] = sum_l x[b, l, c] * mask[b, l] / max(sum_l mask[b, l], 1e-9)
 * x bf16 (fp32 when x_f32) at x + b*x_stride_b + l*x_stride_l + c; mask fp32 [B, L] contiguous or NULL (all ones); out fp32
 * [B, C] contiguous.  fp32 sums in one fixed order (no atomics): repeated runs are bit-identical.  Rows whose mask is 0 are
 * not read.  C a multiple of 4, strides multiples of 4 elements.
 */
typedef struct {
  const void* x; int64_t x_stride_b, x_stride_l;
  const float* mask;
  float* out;
  int32_t B, L, C;
  int32_t x_f32;
} AptpMaskedMeanParams;

int aptp_masked_mean(const AptpMaskedMeanParams* p, aptp_stream_t stream);

/* Fused tail of a transformer block on the large-M levels (diffusers BasicTransformerBlock.norm3 -> ff (GEGLUGated +
 * Linear, pdm/models/unet/blocks.py:41-50,121-129,821-823) -> "+ hidden_states", then Transformer2DModel.proj_out and its
 * "+ residual", blocks.py:1294-1308) as ONE kernel per 64-token tile:
 *   y = proj_out(h + ff2(GEGLU(LN3(h) W1'))) + x,   optionally with the column statistics of y for the next GroupNorm
 * (colstat [M/64][colstat_ld][2] = per (64-row block, channel) (sum, sumsq) of the bf16 outputs: AptpGroupNormParams.colstats
 * with rows_per_block = 64).  w1 = the GEGLU projection packed with the LayerNorm folded in and (value | gate) rows interleaved
 * in blocks of 16 (ops.pack_weight(geglu=True, ln_gamma=, ln_beta=)), b1 its bias', cs1 its column sums; w2 = ff.net[2] packed
 * [C][ld2]; w3 = proj_out packed [C][ld3].  Requires aptp_ff_tail_supported(...) != 0 (M % 64 == 0, C in {64..320} a multiple
 * of 64, ld1 == ld3 == C, ld2 % 64 == 0, n1 % 32 == 0). */
typedef struct {
  const void* h; int64_t ldh;      /* bf16 [M, C]: the residual stream after the cross-attention */
  const void* x; int64_t ldx;      /* bf16 [M, C]: the transformer's input (residual of proj_out) */
  void* y; int64_t ldy;            /* bf16 [M, C] */
  const void* w1; const float* b1; const float* cs1; int32_t n1, ld1;
  const void* w2; const float* b2; int32_t ld2;
  const void* w3; const float* b3; int32_t ld3;
  float* colstat; int32_t colstat_ld;
  int32_t M, C;
  float eps;
} AptpFfTailParams;
int aptp_ff_tail_supported(int M, int C, int n1, int ld1, int ld2, int ld3);
int aptp_ff_tail(const AptpFfTailParams* p, aptp_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Backward path (data gradients + gate gradients; the U-Net weights are frozen in APTP's pruning step,
 * pdm/training/trainer.py:742,827-829).  Data gradients of convolutions / linears reuse aptp_conv_gemm with
 * flipped-transposed packed weights (ups = 2 for the stride-2 downsamplers).  What autograd derives in the reference
 * from F.group_norm / F.silu / F.layer_norm / F.gelu / SDPA / the gate multiplies (blocks.py:41-50,250-260,296-359,
 * 782-821; gates.py:15-21) is implemented by the entry points below.
 * ------------------------------------------------------------------------------------------------------------------- */

/* Width-gate backward: dx = dy * gate[b % gate_B, c / (C/groups)];  dgate_partial[b, chunk, g] = sum over the rows of the
 * chunk and the channels of group g of dy * y0 (y0 = the pre-gate activation).  nchunk = aptp_groupnorm_nchunk(HW); the caller
 * sums the chunk axis (and the CFG-tiled batch rows that share a gate row). */
typedef struct {
  const void* dy; int64_t lddy;   /* bf16 [B*HW, C] */
  const void* y0; int64_t ldy0;   /* bf16 [B*HW, C] */
  void* dx; int64_t lddx;         /* bf16 [B*HW, C] */
  int32_t B, HW, C, groups;
  const float* gate; int32_t gate_B;   /* fp32 [gate_B, groups] */
  float* dgate_partial;                /* fp32 [B, nchunk, groups] */
  float* dgate;                        /* optional fp32 [gate_B, groups]: the partials folded over the chunk axis and over
                                          the batch rows that share a gate row (b = rep*gate_B + bg), fixed order */
} AptpGateBwdParams;
int aptp_gate_bwd(const AptpGateBwdParams* p, aptp_stream_t stream);

/* GEGLU in its training form (value | gate halves side by side, not interleaved): forward out = (h*m) * gelu_erf(g*m);
 * backward (backward = 1): dhg = [dh | dg], dgate_partial[b, chunk, grp] (blocks.py:41-50 through autograd). */
typedef struct {
  const void* hg; int64_t ldhg;        /* bf16 [B*HW, 2C] : h = cols [0,C), g = cols [C,2C) */
  void* out; int64_t ldout;            /* bf16 [B*HW, C]  (forward) */
  const void* dout; int64_t lddout;    /* bf16 [B*HW, C]  (backward) */
  void* dhg; int64_t lddhg;            /* bf16 [B*HW, 2C] (backward) */
  int32_t B, HW, C, groups;
  const float* gate; int32_t gate_B;   /* fp32 [gate_B, groups] or NULL (mask == 1) */
  float* dgate_partial;                /* fp32 [B, nchunk, groups] (backward) */
  int32_t backward;
  float* dgate;                        /* optional fp32 [gate_B, groups] (backward): folded partials, as in AptpGateBwdParams */
} AptpGegluParams;
int aptp_geglu(const AptpGegluParams* p, aptp_stream_t stream);

/* DepthGate in its training form (pdm/models/unet/gates.py:36-42): forward y = (1 - d[b % d_B]) * x_in + d[b % d_B] * x_out;
 * backward (backward = 1): d_out = dy * d, d_in = dy * (1 - d), dd[bg] = sum over the samples that share gate row bg and over
 * all elements of dy * (x_out - x_in) (two-stage, deterministic; dd_partial: fp32 [B, aptp_groupnorm_nchunk(HW)] scratch).
 * In the reference this is five elementwise passes forward and autograd's chain backward; here one launch each way. */
typedef struct {
  const void* x_in; int64_t ld_in;     /* bf16 [B*HW, C] */
  const void* x_out; int64_t ld_out;   /* bf16 [B*HW, C] */
  void* y; int64_t ld_y;               /* bf16 [B*HW, C]  (forward) */
  const void* dy; int64_t ld_dy;       /* bf16 [B*HW, C]  (backward) */
  void* d_in; int64_t ld_d_in;         /* bf16 [B*HW, C]  (backward) */
  void* d_out; int64_t ld_d_out;       /* bf16 [B*HW, C]  (backward) */
  int32_t B, HW, C;
  const float* d; int32_t d_B;         /* fp32 [d_B] */
  float* dd_partial;                   /* fp32 [B, nchunk] (backward) */
  float* dd;                           /* fp32 [d_B] (backward) */
  int32_t backward;
} AptpDepthLerpParams;
int aptp_depth_lerp(const AptpDepthLerpParams* p, aptp_stream_t stream);

/* Weight gradient of a stride-1 "same" convolution (3x3, pad 1) or of a 1x1 convolution / linear layer, for the expert
 * fine-tune step (pdm/training/trainer.py:1616, loss.backward through F.conv2d / F.linear of the pruned expert):
 *   dw[s][n][tap][c] = sum over the pixels m of slice s of dy[m][n] * x[pix(m, tap)][c]      (fp32, packed-weight order)
 * The caller sums the split_m slabs (fixed order: deterministic).  Operands stay in their forward layout: no im2col and no
 * transposed copies; the kernel reads its LDS tiles K-major with gfx950's transposed LDS read.
 * aptp_conv_wgrad_supported: 1 when the geometry is handled (KH == KW in {1, 3}; C, N, ld multiples of 8; for 3x3: H*W a
 * multiple of 32 and W a multiple of 32 or a divisor of 32 that is >= 8), else 0 (use the GEMM on transposed copies). */
typedef struct {
  const void* x; int64_t ldx;      /* bf16 [B*H*W, C]: the convolution's input */
  const void* dy; int64_t lddy;    /* bf16 [B*H*W, N]: gradient of its output */
  float* dw;                       /* fp32 [split_m, N, KH*KW, C] */
  int32_t B, H, W, C, N, KH, KW, split_m;
  int32_t ld_dw;                   /* row length of dw's innermost (c) dimension; 0 = C.  With split_m == 1 and ld_dw = cin_pad the
                                      kernel writes straight into a packed-layout gradient (pad columns are not touched) */
  float* db;                       /* optional fp32 [split_m, N]: per-slice column sums of dy = the bias gradient's slabs (the
                                      workgroups of input-channel block 0 sum the dy tiles they stage anyway) */
  int64_t slab_stride;             /* elements between consecutive slices of dw; 0 = N*KH*KW*ld_dw */
  int64_t db_stride;               /* elements between consecutive slices of db; 0 = N (both non-zero: db rows appended to dw's slabs) */
  /* resampling 3x3 convolutions (Downsample2D / Upsample2D of the U-Net).  H, W above are always the OUTPUT map (the one dy
   * lives on).  stride 2 (0 and 1 both mean 1): x is [B, 2H, 2W, C], pad 1.  ups 1: the convolution reads the nearest-x2
   * up-sampled input: x is [B, H/2, W/2, C].  Not both. */
  int32_t stride, ups;
} AptpWgradParams;
int aptp_conv_wgrad_supported(const AptpWgradParams* p);
int aptp_conv_wgrad_suggest_split(const AptpWgradParams* p);
int aptp_conv_wgrad(const AptpWgradParams* p, aptp_stream_t stream);

/* Every stride-1 weight gradient of a backward pass as ONE launch per filter size (round 3; replaces 225 + 43 per-layer launches
 * of the expert fine-tune step, i.e. F.conv2d / F.linear weight gradients of trainer.py:1616 issued when the backward is
 * complete).  Per item the caller chooses split_m for the BATCH (a pixel slice only has to be worth a workgroup, not to fill the
 * chip: ~2,048 pixels), fills one descriptor of aptp_conv_wgrad_many_item_bytes() bytes with aptp_conv_wgrad_many_fill (host
 * memory; first_block = sum of aptp_conv_wgrad_many_blocks() of the items before it), uploads the descriptor table (16-byte
 * aligned) and an int32 map block -> item of total_blocks entries, and launches.  All items of one call share `taps` (1 or 9);
 * results, slabs and bias-gradient slabs exactly as aptp_conv_wgrad with the same split_m (bit-identical). */
int64_t aptp_conv_wgrad_many_item_bytes(void);
int aptp_conv_wgrad_many_blocks(const AptpWgradParams* p);
int aptp_conv_wgrad_many_fill(const AptpWgradParams* p, void* item_out, int32_t first_block);
int aptp_conv_wgrad_many(const void* items_dev, const int32_t* block_item_dev, int32_t n_items, int32_t total_blocks,
                         int32_t taps, aptp_stream_t stream);

/* out[row][c] = sum over r < R of partials[r][row][c] (partials: fp32 [R][n_rows][C] contiguous; out: fp32 [n_rows][ld_out]); fixed order.
 * The slab sum of a split weight gradient (written into the padded packed layout) and the chunk sums of bias / affine gradients. */
typedef struct {
  const float* partials; float* out; int32_t R, n_rows, C, ld_out;
  float* tail_out; int32_t tail_rows;   /* optional: the LAST tail_rows of the n_rows go to tail_out (fp32 [tail_rows][C], contiguous)
                                           instead of out -- a weight gradient's slabs and its bias gradient's slabs in one fold */
  int32_t pair_split;                   /* 1 (n_rows == 1, C even): the columns are (a, b) pairs -- the (dbeta, dgamma) partials of the norm
                                           backward kernels -- and out receives a_k at [k], b_k at [ld_out + k]: two contiguous
                                           parameter gradients without a strided copy each; b goes to tail_out when that is set (two separate gradient
                                           tensors), else to out + ld_out (>= C/2) */
  int32_t tail_n;                       /* 0 = every tail value; otherwise only the first tail_n of the tail_rows * C tail values are written
                                           (a bias gradient of N values whose slabs were padded to whole rows of C) */
} AptpFoldRowsParams;
int aptp_fold_rows(const AptpFoldRowsParams* p, aptp_stream_t stream);
/* many folds as ONE launch: items_dev = n_items parameter blocks in DEVICE memory (each valid for aptp_fold_rows), starts_dev =
 * n_items + 1 int32 prefix sums of aptp_fold_rows_blocks() (starts[n_items] = total_blocks).  The expert fine-tune step folds the
 * slabs of every split weight gradient this way after its backward (FineTuner.step, trainer.py:1616). */
int aptp_fold_rows_blocks(const AptpFoldRowsParams* p);
int aptp_fold_rows_many(const AptpFoldRowsParams* items_dev, const int32_t* starts_dev, int32_t n_items, int32_t total_blocks,
                        aptp_stream_t stream);

/* AdamW (torch.optim.AdamW arithmetic: decoupled weight decay, bias correction, fp32) over many tensors in ONE launch, writing
 * the bf16 operand the GEMM kernels read in the same pass (the optimizer step of FineTuner.step, pdm/training/trainer.py:1529-1540,
 * 1616-1619).  items_dev: n_items descriptors in DEVICE memory; p, g, m, v 16-byte aligned fp32 [n]; shadow optional bf16 [n]
 * (8-byte aligned).  starts_dev: int32 [n_items + 1] prefix sums of aptp_adamw_blocks(n) in device memory; total_blocks =
 * starts[n_items].  step_dev: fp32 device scalar = number of steps taken before this one (the caller increments it). */
typedef struct { float* p; const float* g; float* m; float* v; void* shadow; int64_t n; } AptpAdamWItem;
typedef struct {
  const AptpAdamWItem* items_dev; const int32_t* starts_dev; int32_t n_items, total_blocks;
  float lr, beta1, beta2, eps, weight_decay;
  const float* step_dev;
  const float* gate_dev;  /* optional fp32 device scalar (e.g. the step's total loss): the launch is a no-op unless it is finite --
                           * the batch-skip of pdm/training/trainer.py:921-929 for a replayed graph; the caller advances step_dev
                           * by the same predicate */
  float grad_scale;       /* gradients are multiplied by this before use (0 = 1): 1 / world size folds the mean of a summed
                           * data-parallel exchange (DDP inside accelerator.backward, trainer.py:1616) into the optimizer pass */
  float warmup_steps;     /* 0 = off; W > 0: the effective rate is lr * min(1, step_dev[0] / W) -- `constant_with_warmup` of
                           * configs/finetuning/sd-2-1_cc3m.yaml:108-109 counted in optimizer steps: the first step runs at rate 0,
                           * step W and later at lr; read from device memory, so a gated (skipped) step does not advance the ramp */
} AptpAdamWParams;
int aptp_adamw_blocks(int64_t n);
int aptp_adamw_many(const AptpAdamWParams* p, aptp_stream_t stream);
/* The same launch with one more factor on the gradients, read from DEVICE memory: grad_scale_dev is an optional fp32 device scalar
 * (4-byte aligned), e.g. the clip coefficient aptp_grad_norm left in out_dev[1]; the gradients are multiplied by
 * grad_scale * grad_scale_dev[0], one fp32 product, uniform over the grid.  Null: aptp_adamw_many itself, bit for bit.  (An
 * argument, not a field: the layout of AptpAdamWParams ends with warmup_steps and stays as it is.) */
int aptp_adamw_many_scaled(const AptpAdamWParams* p, const float* grad_scale_dev, aptp_stream_t stream);
/* The same launch with the RATE read from device memory: lr_dev is an optional fp32 device scalar (4-byte aligned), what
 * aptp_lr_schedule stored for this step.  With it the kernel uses lr_dev[0] where it otherwise forms lr * min(1, step / W): p->lr
 * is ignored, p->warmup_steps != 0 is APTP_EINVAL (the schedule owns the warm-up), one more uniform scalar load and no bytes per
 * element.  Null: aptp_adamw_many_scaled itself, bit for bit (it forwards here).  An argument, not a field, for the same reason. */
int aptp_adamw_many_lr(const AptpAdamWParams* p, const float* grad_scale_dev, const float* lr_dev, aptp_stream_t stream);

/* The same step with both moments kept as block-wise 8-bit codes (csrc/optim8.hip; `use_8bit_adam` of the fine-tune recipe,
 * configs/finetuning/sd-2-1_cc3m.yaml:102; the format is defined by tests/adamw8_model.py).  A quantisation block is
 * 256 consecutive elements of one tensor (the last may be short) with one fp32 absmax per moment; a moment is
 * map[code] * absmax, the first through qmap_signed_dev, the second through qmap_unsigned_dev (256 ascending fp32 each, device
 * memory).  One launch: dequantise, the AdamW element of aptp_adamw_many on p (from the unquantised new moments) and the bf16
 * operand, then absmax = max |.| per block and a nearest code of x / absmax per element.  absmax == 0 stores the zero code
 * throughout; a block with a non-finite new moment stores a NaN absmax.  m8, v8: uint8 [n], 4-byte aligned; absmax_m, absmax_v:
 * fp32 [ceil(n / 256)], 4-byte aligned; p, g, shadow, starts_dev, step_dev, gate_dev, grad_scale, warmup_steps and grad_scale_dev
 * as in aptp_adamw_many_scaled; aptp_adamw8_blocks(n) == aptp_adamw_blocks(n).  items_host: optional host copy of the table;
 * when given, every item is checked (non-null, n >= 1, alignment, block count) before anything is launched.  APTP_EINVAL and
 * nothing launched for: null table, maps or step_dev, n_items / total_blocks < 1, bad hyper-parameters, a misaligned item. */
typedef struct {
  float* p; const float* g; uint8_t* m8; uint8_t* v8; float* absmax_m; float* absmax_v; void* shadow; int64_t n;
} AptpAdamW8Item;
typedef struct {
  const AptpAdamW8Item* items_dev; const int32_t* starts_dev; int32_t n_items, total_blocks;
  float lr, beta1, beta2, eps, weight_decay;
  const float* step_dev;
  const float* gate_dev;
  float grad_scale;
  float warmup_steps;
  const float* qmap_signed_dev;    /* 256 ascending fp32 in [-1, 1], zero at code 127: the first moment's map */
  const float* qmap_unsigned_dev;  /* 256 ascending fp32 in [0, 1], zero at code 0: the second moment's map */
  const AptpAdamW8Item* items_host;
} AptpAdamW8Params;
int aptp_adamw8_blocks(int64_t n);
int aptp_adamw8_many(const AptpAdamW8Params* p, const float* grad_scale_dev, aptp_stream_t stream);
/* lr_dev as in aptp_adamw_many_lr; null: aptp_adamw8_many itself, bit for bit (it forwards here) */
int aptp_adamw8_many_lr(const AptpAdamW8Params* p, const float* grad_scale_dev, const float* lr_dev, aptp_stream_t stream);

/* Gradient accumulation over the micro-batches of one optimizer window (gradient_accumulation_steps of the fine-tune recipe,
 * configs/finetuning/sd-2-1_cc3m.yaml): ONE launch over a contiguous fp32 range (the gradient arena of
 * PackedTrainer.ensure_grad_buffers(arena=True)).  acc, g: fp32 [n], 16-byte aligned; plain fp32 addition, no gate: a
 * non-finite value propagates into the sum.
 *   STORE  acc[i] = g[i]            first micro-step: acc is not read, so it needs no zero fill    (8 B / element)
 *   ADD    acc[i] = acc[i] + g[i]   micro-steps in between                                         (12 B / element)
 *   FINAL  g[i]   = acc[i] + g[i]   last micro-step: the sum lands where the exchange and AdamW read (12 B / element) */
enum { APTP_GRAD_ACCUM_STORE = 0, APTP_GRAD_ACCUM_ADD = 1, APTP_GRAD_ACCUM_FINAL = 2 };
typedef struct { float* acc; float* g; int64_t n; int32_t mode; } AptpGradAccumParams;
int aptp_grad_accumulate_blocks(int64_t n);   /* grid of the launch: 0 for n <= 0 */
int aptp_grad_accumulate(const AptpGradAccumParams* p, aptp_stream_t stream);

/* Exponential moving average of the trained weights over many tensors in ONE launch (csrc/ema.hip; `use_ema` of the reference's
 * interface, pdm/utils/arg_utils.py:50-54, with the decay rule of diffusers' EMAModel).  items_dev: n_items descriptors in DEVICE
 * memory; p, ema 16-byte aligned fp32 [n]; shadow optional bf16 [n] (8-byte aligned).  starts_dev: int32 [n_items + 1] prefix
 * sums of aptp_adamw_blocks(n) in device memory; total_blocks = starts[n_items].
 *   UPDATE  no-op unless gate_dev is null or gate_dev[0] is finite (the predicate of aptp_adamw_many); else, in fp32,
 *             n = count_dev[0] + 1;  s = max(0, n - update_after_step - 1)
 *             d = 0 when s <= 0, else max(min_decay, min(base, decay)) with
 *             base = use_warmup ? 1 - (1 + s / inv_gamma)^(-power) : (1 + s) / (10 + s)
 *             ema <- ema - (1 - d) * (ema - p)   (d = 0 stores p itself); p is read only, shadow ignored; cur_decay_dev[0] <- d
 *           count_dev: fp32 device scalar = EMA steps applied BEFORE this call (the caller advances it by the same predicate).
 *   SWAP    p <-> ema element by element, shadow <- bf16(new p) with the rounding of the AdamW pass; ungated, no count: two
 *           swaps restore every bit of p, ema and shadow.
 * APTP_EINVAL and nothing launched for: null tables, n_items or total_blocks < 1, another mode, UPDATE without count_dev, decay
 * outside [0, 1], min_decay outside [0, decay], update_after_step < 0, inv_gamma <= 0, power <= 0. */
enum { APTP_EMA_UPDATE = 0, APTP_EMA_SWAP = 1 };
typedef struct { float* p; float* ema; void* shadow; int64_t n; } AptpEmaItem;
typedef struct {
  const AptpEmaItem* items_dev; const int32_t* starts_dev; int32_t n_items, total_blocks;
  int32_t mode;
  const float* count_dev;
  const float* gate_dev;     /* optional fp32 device scalar, e.g. the step's total loss */
  float decay, min_decay;
  int32_t update_after_step, use_warmup;
  float inv_gamma, power;
  float* cur_decay_dev;      /* optional fp32 device scalar: written by an applied UPDATE */
} AptpEmaParams;
int aptp_ema_many(const AptpEmaParams* p, aptp_stream_t stream);

/* AdamW over many small fp32 tensors with everything a schedule changes in DEVICE memory (csrc/router_optim.hip): the router's
 * optimizer of a captured pruning step (pdm/training/trainer.py:804-834, 913-933; configs/pruning/sd-2-1_cc3m.yaml).  The
 * arithmetic per element is aptp_adamw_many's, with
 *   t      = step[0] + 1                              the ITEM's own count of applied steps (torch keeps one per parameter and
 *                                                     skips a parameter without a gradient)
 *   lr_eff = lr_g * min(1, applied / warmup_steps_g)  when warmup_steps_g > 0: `constant_with_warmup` counted in applied steps
 * items_dev: n_items descriptors in device memory; p, g, m, v fp32 [n], 16-byte aligned; step: fp32 device scalar; group: index
 * into groups_dev.  starts_dev: int32 [n_items + 1] prefix sums of aptp_group_adamw_blocks(n); total_blocks = starts[n_items].
 * groups_dev: n_groups entries the host may rewrite between replays of a captured launch -- or aptp_lr_schedule, launched in
 * front with out_stride = 3, rewrites the lr column from counters_dev[0] at every step (warmup_steps_g is then 0).
 * counters_dev: fp32 [4], 16-byte aligned = {applied steps, skipped steps, bad-gradient flag (0 outside the call), reserved}.
 * The step is SKIPPED when gate_dev[0] is non-finite or any gradient element of any item is non-finite (NaN or +-Inf; the
 * reference's anomaly mode raises on NaN only): p, m, v, every step[0] and applied keep their bits and skipped advances by 1;
 * otherwise every step[0] and applied advance by 1.  zero_grad != 0: the gradients are written to zero in both cases.
 * Three launches on `stream`: scan, update, advance.  items_host: optional host copy of the table; when given, every item is
 * checked (non-null, n >= 1, group in range, alignment, block count) before anything is launched.  APTP_EINVAL and nothing
 * launched for: null pointers, n_items / n_groups / total_blocks < 1, betas outside [0, 1), eps <= 0, grad_scale < 0, a
 * misaligned table or item. */
typedef struct { float* p; float* g; float* m; float* v; float* step; int64_t n; int32_t group; } AptpGroupAdamWItem;
typedef struct { float lr, weight_decay, warmup_steps; } AptpAdamWGroup;
typedef struct {
  const AptpGroupAdamWItem* items_dev; const int32_t* starts_dev; int32_t n_items, total_blocks;
  const AptpAdamWGroup* groups_dev; int32_t n_groups;
  float* counters_dev;
  float beta1, beta2, eps;
  float grad_scale;       /* gradients are multiplied by this before use (0 = 1); the scan looks at the unscaled values */
  int32_t zero_grad;
  const float* gate_dev;  /* optional fp32 device scalar, e.g. the step's total loss */
  const AptpGroupAdamWItem* items_host;
  const float* grad_scale_dev; /* optional fp32 device scalar (4-byte aligned), e.g. the clip coefficient aptp_grad_norm left in
                           * out_dev[1]: the gradients are multiplied by grad_scale * grad_scale_dev[0], one fp32 product, uniform
                           * over the grid; null: by grad_scale alone, every bit as without the field */
} AptpGroupAdamWParams;
int aptp_group_adamw_blocks(int64_t n);
int aptp_group_adamw(const AptpGroupAdamWParams* p, aptp_stream_t stream);

/* The rate of the next optimizer step from the count of applied steps, on the device (csrc/lr_schedule.hip): the
 * `lr_scheduler` family of the recipes (transformers.optimization.get_scheduler) for the three AdamW kernels above.  ONE launch of
 * one small block; put it in front of the AdamW launch(es) of the step.  With k = count_dev[0], W = warmup_steps, T = training_steps
 * (optimizer steps), the step that follows k applied ones runs at base * m(k); m in fp64:
 *   every kind but CONSTANT, k < W:  m = k / max(1, W)
 *   CONSTANT                         m = 1
 *   CONSTANT_WITH_WARMUP             m = 1 for k >= W
 *   LINEAR                           m = max(0, (T - k) / max(1, T - W))
 *   COSINE                           m = max(0, 0.5 (1 + cos(pi num_cycles 2 prog))), prog = (k - W) / max(1, T - W); it rises again past T
 *   COSINE_WITH_RESTARTS             m = 0 for prog >= 1, else max(0, 0.5 (1 + cos(pi ((num_cycles prog) mod 1))))
 *   POLYNOMIAL                       m = lr_end / lr_init for k > T, else ((lr_init - lr_end) (1 - (k - W) / (T - W))^power + lr_end) / lr_init
 * out_dev[i * out_stride] = (float)((double)base_dev[i] * m) for i < n, except that CONSTANT stores base_dev[i] itself and
 * CONSTANT_WITH_WARMUP the fp32 expression of AptpAdamWParams.warmup_steps, base * min(1, k / W): the same bits as the paths
 * without this launch.  out_stride = 3 writes the lr column of an AptpAdamWGroup table in place (its warmup_steps column must
 * then be 0).  mult_dev: optional, receives (float)m.  lr_init is the OPTIMIZER's default rate, not a group's (the library divides
 * by optimizer.defaults["lr"]; the reference builds its optimizers from groups, so that is torch.optim.AdamW's 1e-3).
 * APTP_EINVAL and nothing launched for: null or misaligned count_dev / base_dev / out_dev, a misaligned mult_dev, an unknown kind,
 * negative steps or steps >= 2^24 (k is an fp32 count), T < W for the four decaying kinds (T <= W for POLYNOMIAL), n outside
 * 1..16, out_stride < 1, and for the kinds that read them num_cycles <= 0, power <= 0, lr_init <= lr_end. */
enum {
  APTP_LR_CONSTANT = 0, APTP_LR_CONSTANT_WITH_WARMUP = 1, APTP_LR_LINEAR = 2, APTP_LR_COSINE = 3,
  APTP_LR_COSINE_WITH_RESTARTS = 4, APTP_LR_POLYNOMIAL = 5
};
typedef struct {
  int32_t kind;
  int32_t warmup_steps, training_steps;
  int32_t n;                   /* rates to write: 1 <= n <= 16 */
  double num_cycles;           /* COSINE (0.5 = half a wave down to 0 at T), COSINE_WITH_RESTARTS (an integer) */
  double power, lr_end, lr_init; /* POLYNOMIAL */
  const float* count_dev;      /* fp32 device scalar: applied steps (PackedAdamW.step_t, RouterAdamW.counters[0]) */
  const float* base_dev;       /* n base rates */
  float* out_dev;              /* element i at out_dev[i * out_stride] */
  int32_t out_stride;
  float* mult_dev;             /* optional */
} AptpLrScheduleParams;
int aptp_lr_schedule(const AptpLrScheduleParams* p, aptp_stream_t stream);

/* Global L2 norm of the gradients of a table and the clip coefficient of torch.nn.utils.clip_grad_norm_ (max_grad_norm), both left
 * in device memory (csrc/grad_norm.hip): what grad_scale_dev of aptp_adamw_many_scaled and aptp_group_adamw reads.  items_dev: n_items
 * descriptors in DEVICE memory, g fp32 [n], 16-byte aligned.  starts_dev: int32 [n_items + 1] prefix sums of
 * aptp_grad_norm_blocks(n) (= aptp_adamw_blocks(n)); total_blocks = starts[n_items].  Two launches on `stream`, no atomics, fp64
 * accumulation in a FIXED order, so the four floats are the same bits at every replay:
 *   partial   one block of 256 threads per 4096 elements of an item; thread t, trips i = 0..3 at e = base + (i * 256 + t) * 4:
 *             s += (double)g * (double)g over g[e], g[e+1], g[e+2], g[e+3] (or the item's last 1..3 elements) in index order;
 *             per wave of 64 a butterfly s = s + s[lane ^ off], off = 32, 16, 8, 4, 2, 1; then ((w0 + w1) + w2) + w3 -> partials[b]
 *   finalise  one block: thread j adds partials[j], partials[j + 256], ... in that order, the same tree gives S; then in fp64
 *             total = sqrt(S) * grad_scale;  r = max_norm / (total + 1e-6);  coef = r < 1 ? max(r, 0) : 1, rounded to fp32
 *             (so 1.0f for a null max_norm_dev, +inf, or total <= max_norm - 1e-6)
 *             verdict = (float)total when it and gate_dev[0] (when given) are finite, else NaN -- and then coef = 1.0f
 *             clipped_count += 1 when the verdict is finite and coef < 1
 * out_dev: fp32 [4] = {total_norm, clip_coef, verdict, clipped_count}; the caller zeroes clipped_count once.
 * APTP_EINVAL and nothing launched for: null items_dev / starts_dev / partials_dev / out_dev, n_items or total_blocks < 1,
 * grad_scale < 0, out_dev not 16-byte or partials_dev not 8-byte aligned. */
typedef struct { const float* g; int64_t n; } AptpGradNormItem;
typedef struct {
  const AptpGradNormItem* items_dev; const int32_t* starts_dev; int32_t n_items, total_blocks;
  double* partials_dev;        /* [total_blocks] scratch; every slot is written */
  float   grad_scale;          /* 0 = 1: the scale the optimizer will apply (1 / micro-batches, 1 / world) */
  const float* max_norm_dev;   /* optional fp32 device scalar > 0; null or +inf = measure only, coef = 1 */
  const float* gate_dev;       /* optional fp32 device scalar (the loss) */
  float* out_dev;
} AptpGradNormParams;
int aptp_grad_norm_blocks(int64_t n);
int aptp_grad_norm(const AptpGradNormParams* p, aptp_stream_t stream);

/* Mean squared error of two equally shaped activations, read where they lie (the loss terms of Pruner.step / FineTuner.step:
 * pdm/training/trainer.py:1197-1225 diffusion MSE, output distillation, block distillation; :1729-1752 for the fine-tune step).
 * backward = 0: out[0] = mean((a - b)^2); partial: fp32 [aptp_mse_nblocks(rows, C)] scratch (every slot is written).
 * backward = 1: da = (a - b) * g[0] * 2 / (rows * C)   (g: the fp32 device scalar dL/d(out); da has a's element type).
 * f32 = 0: bf16 operands; f32 = 1: fp32 operands.  C multiple of 8; leading dimensions in elements, multiples of 8. */
typedef struct {
  const void* a; int64_t lda;
  const void* b; int64_t ldb;
  int64_t rows; int32_t C; int32_t f32;
  float* partial; float* out;
  const float* g; void* da; int64_t ldda;
  int32_t backward;
} AptpMseParams;
int aptp_mse_nblocks(int64_t rows, int32_t C);
int aptp_mse(const AptpMseParams* p, aptp_stream_t stream);

/* Every loss term of one validation step at once (Pruner.validate / FineTuner.validate: pdm/training/trainer.py:1026-1095,
 * 1767-1818), with running totals kept on the device: three launches, no atomics, nothing to zero per call.
 * A term is mean((a - b)^2) of two equally shaped operands read where they lie, with the operand rules of AptpMseParams and a
 * dtype flag PER OPERAND (a bf16 activation against an fp32 target needs no cast).
 *   rows_per_sample = 0: one mean over the whole term.
 *   rows_per_sample > 0: B = rows / rows_per_sample per-sample means m_b; the term's value is (1/B) sum_b w[b] * m_b, summed in
 *                        fp32 in sample order (the min-SNR diffusion term, trainer.py:1736-1749).  At most one such term.
 * Every unweighted term gets the workgroups, the grid stride, the in-block fold and the finish order aptp_mse gives the same
 * view, and so does every sample of the weighted term: these values are bit-identical to aptp_mse's.
 *   out[g]  = (sum over the terms of group g, in index order, of value * scale), divided by group_div[g] where that is not 0
 *             (the training step's block loss is (m_1 + .. + m_9) / 9: scale 1 and group_div 9 give its bits, scale 1/9 does not)
 *   out[G]  = sum_g group_coef[g] * out[g], in index order     (G = n_groups; out: fp32 [G + 1], written on every call)
 *   sample_out (optional): fp32 [B], the per-sample means of the weighted term
 *   running (optional): fp32 [G + 2]; running[g] += out[g] for g = 0..G and running[G + 1] += 1, by one thread.  The caller
 *             zeroes it once per validation run.  Non-finite values pass through.
 * partial: fp32 [aptp_loss_terms_scratch_floats(p)] scratch, every slot that is read is written first. */
#define APTP_LOSS_TERMS_MAX 16
typedef struct {
  const void* a; int64_t lda;
  const void* b; int64_t ldb;
  int64_t rows; int64_t rows_per_sample;
  int32_t C; int32_t a_f32; int32_t b_f32; int32_t group;
  float scale; int32_t reserved;
} AptpLossTerm;
typedef struct {
  AptpLossTerm terms[APTP_LOSS_TERMS_MAX];
  int32_t n_terms; int32_t n_groups;
  float group_coef[APTP_LOSS_TERMS_MAX];
  float group_div[APTP_LOSS_TERMS_MAX];
  const float* w;
  float* partial; float* out; float* sample_out; float* running;
} AptpLossTermsParams;
int aptp_loss_terms_nblocks(const AptpLossTermsParams* p);          /* workgroups of the first launch: the sum of aptp_mse_nblocks
                                                                      over the terms and samples; 0 for a table it would refuse */
int aptp_loss_terms_scratch_floats(const AptpLossTermsParams* p);   /* those partials plus one value per term / sample */
int aptp_loss_terms(const AptpLossTermsParams* p, aptp_stream_t stream);

/* The loss stage of a TRAINING step whose batch may be short (FineTuner.step, pdm/training/trainer.py:1736-1763, on a batch
 * from which collate_fn dropped samples, pdm/utils/data_utils.py:175-179): every term per sample, a 0 / 1 mask over the
 * samples, the mean over the samples PRESENT, and every gradient from one launch.
 * A term is AptpLossTerm's (operand rules of AptpMseParams, a dtype flag per operand) with rows_per_sample > 0 required:
 * B = rows / rows_per_sample is the same for all terms, 1 <= B <= APTP_LOSS_STAGE_MAX_B.  Unit (t, b) = mean((a - b)^2) over
 * sample b of term t has the workgroups, the grid stride and the folds aptp_mse gives that sample's view: the same bits.
 *   valid: fp32 [B] of 0 and 1 in any pattern; w: fp32 [B], may be null when no term has `weighted` set
 *   n        = sum_b valid[b]
 *   term_t   = (1/n) sum_b valid[b] * (weighted ? w[b] : 1) * unit[t][b], in sample order; samples with valid[b] = 0 are
 *              SKIPPED, not multiplied by 0: what their rows hold (NaN included) reaches no output
 *   out[g]   = (sum over the terms of group g, in index order, of term * scale), / group_div[g] where that is not 0
 *   out[G]   = sum_g group_coef[g] * out[g];  out[G + 1] = n      (out: fp32 [G + 2]; n = 0: all of it 0)
 *   sample_out (optional): fp32 [B], unit[t][b] of the first weighted term (term 0 without one), 0 where valid[b] = 0
 * aptp_loss_stage: three launches (partial, finish, combine), no atomics; partial: fp32 [aptp_loss_stage_scratch_floats(p)].
 * aptp_loss_stage_bwd: ONE launch for the gradients w.r.t. the first operands.  Gradient item i names one or two terms with
 * the SAME first operand (pointer, lda, rows, C, dtype; term1 = -1: one term) and receives
 *   grad_out[b, e] = c_0[b] * (a - b_0) + c_1[b] * (a - b_1),
 *   c_t[b] = g[0] * 2 * group_coef[group_t] * scale_t * valid[b] * (weighted_t ? w[b] : 1) / (n * E_t * gdiv_t)
 * (E_t elements per sample; gdiv_t = group_div[group_t], 1 where that is 0; g: fp32 device scalar, the upstream gradient;
 * c_t is formed in fp64 and rounded once).  grad_out has a's element type, rows of C elements at pitch ldg (0 = lda).  Rows of
 * samples with valid[b] = 0 are WRITTEN as zeros without reading the operands; n = 0 writes zeros everywhere.  n is read from
 * out[G + 1]: call after aptp_loss_stage on the same block.  Nothing outside the C columns of the B * rows_per_sample rows is
 * written.
 * APTP_EINVAL and nothing launched for: null pointers, n_terms / n_groups / n_grads outside 1..16, C no positive multiple of
 * 8, pitches below C or no multiples of 8, operands or grad_out not 16-byte aligned, rows no multiple of rows_per_sample,
 * differing B, B above APTP_LOSS_STAGE_MAX_B, a weighted term with w null, a group or a term index out of range, two terms
 * of an item with different first operands. */
#define APTP_LOSS_STAGE_MAX_B 1024
typedef struct {
  const void* a; int64_t lda;
  const void* b; int64_t ldb;
  int64_t rows; int64_t rows_per_sample;
  int32_t C; int32_t a_f32; int32_t b_f32; int32_t group;
  float scale; int32_t weighted;
} AptpLossStageTerm;
typedef struct {
  void* grad_out; int64_t ldg;
  int32_t term0; int32_t term1;
} AptpLossStageGrad;
typedef struct {
  AptpLossStageTerm terms[APTP_LOSS_TERMS_MAX];
  int32_t n_terms; int32_t n_groups;
  float group_coef[APTP_LOSS_TERMS_MAX];
  float group_div[APTP_LOSS_TERMS_MAX];
  const float* valid; const float* w;
  float* partial; float* out; float* sample_out;
  AptpLossStageGrad grads[APTP_LOSS_TERMS_MAX];
  int32_t n_grads; int32_t reserved;
  const float* g;
} AptpLossStageParams;
int aptp_loss_stage_nblocks(const AptpLossStageParams* p);          /* workgroups of the first launch; 0 for a refused table */
int aptp_loss_stage_scratch_floats(const AptpLossStageParams* p);   /* those partials plus n_terms * B unit values */
int aptp_loss_stage(const AptpLossStageParams* p, aptp_stream_t stream);
int aptp_loss_stage_bwd_nblocks(const AptpLossStageParams* p);      /* workgroups of the gradient launch; 0 for a refused table */
int aptp_loss_stage_bwd(const AptpLossStageParams* p, aptp_stream_t stream);

/* The router's batch-coupled stage of a PRUNING step whose batch may be short (Pruner.step, pdm/training/trainer.py:1129-1249):
 * what couples the samples of a batch outside the U-Net terms, over the samples present.  valid: fp32 [B] of 0 and 1 in any
 * pattern, read at launch time; V = {b: valid[b] != 0}, n = sum_b valid[b].  fp32 throughout, every sum in one fixed order, no
 * atomics: the same bits at every replay.  A sample outside V is skipped, not multiplied by 0: a NaN in its rows reaches nothing.
 *
 * aptp_sinkhorn_assign, ONE launch: the quantiser's Sinkhorn assignment (pdm/models/vq/quantizer.py:263-340) over V.
 *   scores fp32 [B, K] at pitch ld -> idx int64 [B]; q: fp32 [B, K] contiguous, workspace AND output (the transport plan, for
 *   tests).  q = exp(scores / eps) on the rows of V; q /= sum(q); `iters` times: columns (codes) /= their sum over V, /= K, rows
 *   (samples) /= their sum, /= n; q *= n; idx[b] = first argmax_k q[b][k].  A sample outside V -- every sample when n = 0 -- gets
 *   the first argmax of its own raw score row (the quantiser's eval branch: a real code that depends on no other sample) and a
 *   q row of zeros.  A NaN counts as the maximum, as torch.argmax has it.
 *
 * aptp_router_stage, three launches: the contrastive loss (pdm/losses/contrastive_loss.py:5-22) and the MAC losses
 * (trainer.py:1227-1238, pdm/losses/resource_loss.py:5-23) over V.  text fp32 [B, D], arch fp32 [B, E] (row pitches ld_*),
 * ratios fp32 [B].  With Â_i = arch_i / |arch_i|, Ẑ_i = text_i / |text_i|, P = softmax_row(Â Â^T / tau_arch) and
 * T = softmax_row(Ẑ Ẑ^T / tau_text) over V x V, rbar / rmax / sd the mean, maximum and unbiased deviation of ratios over V:
 *   out[0] contrastive = -(1/n^2) sum_{i,j in V} [T_ij log P_ij + (1 - T_ij) log(1 - P_ij)], each log clamped at -100; where
 *          P_ij > 1/2, 1 - P_ij is formed from the other exponentials of the row
 *   out[1] resource    = LOG: log(rbar > p ? rbar / p : p / rbar);  MAE: |rbar - p|;  MSE: (rbar - p)^2
 *   out[2] max_loss    = 1 - rmax
 *   out[3] std_loss    = -sd          (n = 1: NaN, as torch.std)
 *   out[4] router_loss = w_resource * out[1] + w_contrastive * out[0] + w_std * out[3] + w_max * out[2], in this order
 *   out[5] rbar;  out[6] n;  out[7] the number of samples of V with ratios == rmax.        n = 0: all eight are 0.
 * aptp_router_stage_bwd, two launches, after aptp_router_stage on the same block: the gradient of g[0] * router_loss (g: fp32
 * device scalar) as d_arch fp32 [B, E] at pitch ld_darch and d_ratios fp32 [B].  BCE backward as torch has it,
 * dP_ij = (P_ij - T_ij) / max(P_ij (1 - P_ij), 1e-12) / n^2; the row-softmax backward; dÂ = (dS + dS^T) Â / tau_arch; the
 * normalisation.  The maximum's gradient is shared evenly among the samples that attain it, the deviation's is 0 where sd is
 * exactly 0 (torch.max, torch.std).  Rows of samples outside V are WRITTEN as zeros without reading the operands.
 * The statistics of the ratios (rbar, sd, the resource term against the fp64 target p) are accumulated in fp64 and rounded once.
 * work: fp32 [aptp_router_stage_work_floats(B, E, D)], written by the forward and read by the backward.
 * APTP_EINVAL and nothing launched (no HIP call is made) for: a null block or pointer, B outside 1..1024, K outside 1..64, E or
 * D outside 1..4096, a pitch below the row length, iters outside 0..1000, eps or a temperature <= 0, an unknown resource type. */
#define APTP_ROUTER_STAGE_MAX_B 1024
#define APTP_ROUTER_STAGE_MAX_FEATURES 4096
#define APTP_SINKHORN_MAX_K 64
enum { APTP_RESOURCE_LOG = 0, APTP_RESOURCE_MAE = 1, APTP_RESOURCE_MSE = 2 };
typedef struct {
  const float* scores; int64_t ld;
  const float* valid;
  int64_t* idx;
  float* q;
  int32_t B, K, iters;
  float eps;
} AptpSinkhornParams;
int aptp_sinkhorn_assign(const AptpSinkhornParams* p, aptp_stream_t stream);
typedef struct {
  const float* text; int64_t ld_text;
  const float* arch; int64_t ld_arch;
  const float* ratios;
  const float* valid;
  const float* g;
  float* work; float* out;
  float* d_arch; int64_t ld_darch;
  float* d_ratios;
  int32_t B, E, D, resource_type;
  float tau_arch, tau_text;
  double p;
  float w_resource, w_contrastive, w_std, w_max;
} AptpRouterStageParams;
int64_t aptp_router_stage_work_floats(int32_t B, int32_t E, int32_t D);    /* 0 for sizes out of range */
int aptp_router_stage(const AptpRouterStageParams* p, aptp_stream_t stream);
int aptp_router_stage_bwd(const AptpRouterStageParams* p, aptp_stream_t stream);

/* The router's Gumbel-sigmoid relaxation in training mode (pdm/models/vq/quantizer.py:196-213) on SEEDED noise: the project's
 * Philox stream instead of the host generator, so a value is a pure function of (seed of the row, draw, element).  The stream,
 * the draw map and the arithmetic are csrc/gumbel_relax.h.  Row r has seed seeds[r] (int64 [R], device); the Philox draw of
 * the call is formed IN THE KERNEL from draw[0] (int64 [1], device): 8 * draw[0] + sub for sample rows (sub = 6: the noise of the
 * optimal-transport assignment, 7: of the relaxation), 2^63 | draw[0] when `codebook` is set (draw[0] is then the count of
 * steps run).  Element e = c for width column c, e = nw + j for the depth entry at SORTED position j.
 *   aptp_gumbel_relax, ONE launch: z fp32 [R, E] -> out fp32 [R, E], E = nw + nd, both contiguous.
 *     width  w = sigmoid((z + G + base) / T); with non_zero_width, a segment [seg_start[s], seg_start[s + 1]) with no
 *            w >= 0.5 gets + 0.5 on its first entry
 *     depth  p = flip(cumsum(softmax(z[nw:]))), x = log(p + 1e-6) - log1p(-(p - 1e-6)), d_sorted = sigmoid((x + G + base) / T),
 *            out[nw + depth_order[j]] = d_sorted[j]
 *   aptp_gumbel_relax_bwd, ONE launch: dout fp32 [R, E] -> dz fp32 [R, E] = d out / d z with the noise and the bump as
 *     constants; z, seeds and draw as the forward had them, everything else is recomputed (out is not read).
 *   aptp_philox_gumbel, ONE launch: out fp32 [R, n] = G of (seeds[r], that draw, offset + i), and / or words uint32 [R, n], the
 *     Philox word behind each value (either pointer may be null, not both).
 * seg_start int32 [n_seg + 1] and depth_order int32 [nd] are DEVICE tables; seg_start_host / depth_order_host are the same
 * values in host memory, read by the validation only.  fp32, every sum in index order, no atomics: the same bits at every replay.
 * APTP_EINVAL and nothing launched (no HIP call is made) for: a null block or pointer, R outside 1..65535, E outside 1..4096,
 * n_seg above 1024 (or 0 with nw > 0), nd above 64, sub outside {6, 7}, T <= 0, a seg_start that does not start at 0, end at nw
 * and strictly increase, a depth_order entry outside [0, nd) or named twice, n outside 1..2^31, offset outside [0, 2^62]. */
#define APTP_GUMBEL_RELAX_MAX_R 65535
#define APTP_GUMBEL_RELAX_MAX_E 4096
#define APTP_GUMBEL_RELAX_MAX_SEG 1024
#define APTP_GUMBEL_RELAX_MAX_ND 64
typedef struct {
  const float* z; float* out;
  const float* dout; float* dz;
  const int64_t* seeds; const int64_t* draw;
  const int32_t* seg_start; const int32_t* depth_order;
  const int32_t* seg_start_host; const int32_t* depth_order_host;
  int32_t R, nw, nd, n_seg;
  int32_t sub, codebook, non_zero_width, reserved;
  float T, base;
} AptpGumbelRelaxParams;
int aptp_gumbel_relax(const AptpGumbelRelaxParams* p, aptp_stream_t stream);
int aptp_gumbel_relax_bwd(const AptpGumbelRelaxParams* p, aptp_stream_t stream);
typedef struct {
  float* out; uint32_t* words;
  const int64_t* seeds; const int64_t* draw;
  int64_t n, offset;
  int32_t R, sub, codebook, reserved;
} AptpPhiloxGumbelParams;
int aptp_philox_gumbel(const AptpPhiloxGumbelParams* p, aptp_stream_t stream);

/* Data-gradient operand from the forward operand of the same contraction (both in packed bf16 layout):
 * dst[c][taps-1-t][n] = src[n][t][c] for n < N, c < C, zero in the rest of dst's [dst_rows][taps][dst_ld] image.
 * (ops.pack_weight_dgrad of the same weights, without going through the diffusers layout.) */
typedef struct { const void* src; void* dst; int32_t N, C, taps, src_ld, dst_ld, dst_rows; } AptpPackDgradParams;
int aptp_pack_dgrad(const AptpPackDgradParams* p, aptp_stream_t stream);
/* The same for many weights in ONE launch (the operand refresh after an optimizer step): items_dev = n_items descriptors in
 * DEVICE memory (each validated by the caller as aptp_pack_dgrad would), starts_dev = int32 [n_items + 1] prefix sums of
 * aptp_pack_dgrad_blocks(item) (device memory), total_blocks = starts[n_items]. */
int aptp_pack_dgrad_blocks(const AptpPackDgradParams* p);
int aptp_pack_dgrad_many(const AptpPackDgradParams* items_dev, const int32_t* starts_dev, int32_t n_items, int32_t total_blocks,
                         aptp_stream_t stream);

/* GroupNorm(+SiLU) data gradient.  fwd_stats = the [B, nchunk, groups, 2] (sum, sumsq) partials the forward wrote into its
 * workspace (keep that buffer alive); workspace: fp32 [B, nchunk, groups, 2]. */
typedef struct {
  const void* x; int64_t ldx;
  const void* dy; int64_t lddy;
  void* dx; int64_t lddx;
  int32_t B, HW, C, groups;
  const float* gamma; const float* beta;
  float eps; int32_t silu;
  const float* fwd_stats;
  void* workspace;
  float* pgrad_partial;   /* optional fp32 [B, nchunk, C, 2]: per-channel (sum dz, sum dz*xhat) -> dbeta, dgamma (fine-tuning) */
  const void* add; int64_t ldadd;   /* optional bf16 [B*HW, C]: dx = (norm gradient) + add in fp32, rounded once -- the gradient that
                                     * arrives over the residual path when x forks into norm(x) and `+ x` (round 3) */
} AptpGroupNormBwdParams;
int aptp_groupnorm_bwd(const AptpGroupNormBwdParams* p, aptp_stream_t stream);

/* LayerNorm data gradient (statistics recomputed from x in registers). */
typedef struct {
  const void* x; int64_t ldx;
  const void* dy; int64_t lddy;
  void* dx; int64_t lddx;
  int32_t rows, C;
  const float* gamma;
  float eps;
  const void* add; int64_t ldadd;   /* optional bf16 [rows, C]: dx += add (as AptpGroupNormBwdParams.add) */
} AptpLayerNormBwdParams;
int aptp_layernorm_bwd(const AptpLayerNormBwdParams* p, aptp_stream_t stream);

/* Column sums of `batch` (0 = 1) consecutive bf16 [rows, C] matrices (bias gradients; batch > 1: per-sample sums for the
 * gradient of a per-sample output bias): partial fp32 [nchunk, batch, C], nchunk = aptp_groupnorm_nchunk(rows) for batch > 1,
 * aptp_rows_nchunk(rows) otherwise. */
typedef struct { const void* x; int64_t ldx; int32_t rows, C; float* partial; int32_t batch; } AptpColsumParams;
int aptp_colsum(const AptpColsumParams* p, aptp_stream_t stream);

/* LayerNorm affine-parameter gradient partials: fp32 [aptp_rows_nchunk(rows), C, 2] = (sum dy, sum dy*xhat). */
typedef struct {
  const void* x; int64_t ldx;
  const void* dy; int64_t lddy;
  int32_t rows, C;
  float eps;
  float* partial;
} AptpLayerNormPgradParams;
int aptp_layernorm_pgrad(const AptpLayerNormPgradParams* p, aptp_stream_t stream);

/* Attention backward: dq, dk, dv from q, k, v, o, dout and the forward's lse; delta is fp32 scratch [B, heads, Lq].
 * Same strided [B, L, heads, 64] layout convention as aptp_attention.  APTP_EINVAL and nothing launched for: null pointers
 * (lse and delta included), extents < 1, a stride that is not a multiple of 8 elements, a pointer that is not 16-byte aligned,
 * a row stride below heads*64, scale <= 0 or NaN, q_split > 1 without an aligned workspace or above ceil(Lq / 64). */
typedef struct {
  const void* q; int64_t q_stride_b, q_stride_l;
  const void* k; int64_t k_stride_b, k_stride_l;
  const void* v; int64_t v_stride_b, v_stride_l;
  const void* o; int64_t o_stride_b, o_stride_l;
  const void* dout; int64_t dout_stride_b, dout_stride_l;
  void* dq; int64_t dq_stride_b, dq_stride_l;
  void* dk; int64_t dk_stride_b, dk_stride_l;
  void* dv; int64_t dv_stride_b, dv_stride_l;
  const float* lse; float* delta;
  int32_t B, heads, Lq, Lk;
  float scale;       /* > 0, the forward's */
  int32_t q_split;  /* dK/dV: split the query range over this many workgroups (0 / 1 = off; aptp_attention_bwd_q_split suggests
                        it: few keys -- cross-attention's 77 -- leave one key tile per (b, head)), fp32 partials folded in slice order */
  void* workspace;   /* aptp_attention_bwd_workspace_bytes(p, q_split) bytes, 16-byte aligned, when q_split > 1 */
} AptpAttentionBwdParams;
int aptp_attention_bwd_q_split(const AptpAttentionBwdParams* p);
size_t aptp_attention_bwd_workspace_bytes(const AptpAttentionBwdParams* p, int32_t q_split);
int aptp_attention_bwd(const AptpAttentionBwdParams* p, aptp_stream_t stream);

/* Image front end of the CLIP image encoder: what cmmd-pytorch/embedding.py:26-30 (_resize_bicubic) and :57-65 (the
 * CLIPImageProcessor call with do_normalize only) do on the host, and the unfold the patch convolution of transformers'
 * CLIPVisionEmbeddings implies, in one launch.  x: fp32 images in [0, 1], [B, H, W, 3] (nchw = 0, CMMD's array format) or
 * [B, 3, H, W] (nchw = 1, the pipeline's "pt" output), any H and W.
 *   resize = 1: bicubic resize to S x S with F.interpolate(mode="bicubic") semantics (A = -0.75, align_corners = False, no
 *               antialiasing, border indices clamped, overshoot not clamped), then (v - mean[c]) / std[c];
 *   resize = 0: x is already preprocessed pixel_values [B, 3, S, S] (nchw = 1, H = W = S) and is only patchified.
 * out: [B * (S/P)^2, ldo] with ldo = ceil(3 P^2 / 64) * 64; row (b, gy, gx) holds patch (gy, gx) of image b in the element order
 * of patch_embedding.weight.flatten(1) (c, py, px), columns [3 P^2, ldo) are written as zeros: the patch convolution is a plain
 * linear layer without bias on these rows.  bf16, or fp32 when out_f32. */
typedef struct {
  const float* x; int32_t nchw;
  int32_t B, H, W;
  int32_t S, P;
  int32_t resize;
  float mean[3], std[3];
  void* out; int64_t ldo;
  int32_t out_f32;
} AptpImagePatchesParams;
int aptp_image_patches(const AptpImagePatchesParams* p, aptp_stream_t stream);

/* CLIPVisionEmbeddings + pre_layrnorm (transformers modeling_clip.py, CLIPVisionTransformer.forward): row 0 of every sample is
 * class_embedding, row 1 + t is row t of the patch GEMM's fp32 output; position_embedding is added and the LayerNorm applied in
 * fp32, with one rounding to the residual stream (bf16, or fp32 when out_f32).  The counterpart of aptp_embed_ln.
 * patches fp32 [B * (T - 1), >= C] (row stride ldp), cls fp32 [C], pos fp32 [T, C], out [B, T, C] (row stride ldo).
 * C a multiple of 8, at most 2048. */
typedef struct {
  const float* patches; int64_t ldp;
  const float* cls; const float* pos; const float* gamma; const float* beta;
  void* out; int64_t ldo;
  int32_t B, T, C;
  int32_t out_f32;
  float eps;
} AptpVitEmbedLnParams;
int aptp_vit_embed_ln(const AptpVitEmbedLnParams* p, aptp_stream_t stream);

/* Rows of an fp32 [n, D] matrix divided by their Euclidean norm (cmmd-pytorch/embedding.py:70, pdm/utils/clip_utils.py:160-161;
 * no epsilon, as there).  D a multiple of 4; x and out may be the same memory. */
typedef struct { const float* x; int64_t ldx; float* out; int64_t ldo; int32_t n, D; } AptpL2NormalizeParams;
int aptp_l2_normalize(const AptpL2NormalizeParams* p, aptp_stream_t stream);

/* The MMD statistic of cmmd-pytorch/distance.py:28-64 with the Gaussian kernel k(a, b) = exp(-|a - b|^2 / (2 sigma^2)):
 *   out[0] = scale * (mean k(x, x) + mean k(y, y) - 2 mean k(x, y))
 * for fp32 x [n, D] and y [m, D].  The Gram tiles (v_mfma_f32_16x16x4_f32: fp32 operands), the squared distances and 1 - k =
 * -expm1(-d^2 / (2 sigma^2)) are formed and summed inside 128 x 128 tiles; no n x n, n x m or m x m matrix is stored.  Every
 * tile writes one fp32 partial to the workspace; one workgroup then adds them in a fixed order in fp64: bit-identical from run to
 * run.  (1 - k is summed rather than k: the result is about 1e-4 of its three terms.)
 * out: fp64 [4] = the statistic, mean(1 - k_xx), mean(1 - k_yy), mean(1 - k_xy).
 * workspace: aptp_mmd_rbf_workspace_bytes(n, m) bytes, 16-byte aligned.  n, m >= 1; D a multiple of 4; ldx, ldy multiples of 4. */
typedef struct {
  const float* x; int64_t ldx;
  const float* y; int64_t ldy;
  int32_t n, m, D;
  float sigma, scale;
  void* workspace;
  double* out;
} AptpMmdRbfParams;
int64_t aptp_mmd_rbf_workspace_bytes(int32_t n, int32_t m);
int aptp_mmd_rbf(const AptpMmdRbfParams* p, aptp_stream_t stream);

/* Image front end of the CLIP score: OpenAI CLIP's `preprocess` (pdm/utils/clip_utils.py:209, :197-221) -- Resize(S, BICUBIC)
 * on a PIL image, CenterCrop(S), ToTensor, Normalize -- on uint8 images x [B, H, W, 3], followed by the unfold of
 * aptp_image_patches (same rows, same zero tail; bf16, or fp32 when out_f32).
 *   size:     the shorter side goes to S, the longer one to (int)(S * long / short)  (aptp_image_patches_pil_size);
 *   resample: PIL's 8-bit bicubic, bit for bit: A = -0.5, support 2 * max(in / out, 1) (antialiased), per output index the window
 *             [xmin, xmin + count) and its normalised weights rounded to 22 fractional bits, the horizontal pass first, each
 *             pass ending in clamp((acc + 2^21) >> 22, 0, 255) stored as uint8; a pass whose size does not change is skipped;
 *   crop:     S x S at top = round((H1 - S) / 2), left likewise, halves to the even neighbour (Python's round);
 *   values:   (u8 / 255 - mean[c]) / std[c] in fp32.
 * The coefficient tables are built by the caller in double precision (ops.pil_bicubic_table) and only read here: the kernels do
 * integer arithmetic.  Per axis: bounds int32 [out, 2] = (xmin, count), weights int32 [out, k] with k the declared window
 * (xk, yk).  A declared window narrower than the resize needs, or an image with a side of 0, is refused with APTP_EINVAL; the
 * kernels additionally clamp every window to the table's k and to the image, so no table can move a read out of range.
 * Two launches: the horizontal pass writes the uint8 scratch image [B, H, W1, 3] (needed when W1 != W), the second launch reads
 * it for the vertical pass, the crop, the normalisation and the unfold.  Tables of a pass that is skipped may be null. */
typedef struct {
  const uint8_t* x;
  int32_t B, H, W;
  int32_t S, P;
  const int32_t* xbounds; const int32_t* xweights; int32_t xk;
  const int32_t* ybounds; const int32_t* yweights; int32_t yk;
  void* scratch;
  float mean[3], std[3];
  void* out; int64_t ldo;
  int32_t out_f32;
} AptpImagePatchesPilParams;
/* the resized extents (H1, W1) and the crop offsets of an H x W image; any of the four pointers may be null */
int aptp_image_patches_pil_size(int32_t H, int32_t W, int32_t S, int32_t* H1, int32_t* W1, int32_t* top, int32_t* left);
int aptp_image_patches_pil(const AptpImagePatchesPilParams* p, aptp_stream_t stream);

/* Pooled output of a CLIP text tower (transformers CLIPTextTransformer.forward, OpenAI encode_text): per prompt the pooling
 * position -- APTP_EOS_ARGMAX: the first index of the largest id; APTP_EOS_FIRST: the first index equal to eos_token_id, 0 when
 * the row has none -- and final_layer_norm of that one row of the residual stream x [B, L, C] (bf16, or fp32 when x_f32; strides
 * in elements), statistics in fp32.  One wave per prompt; the other B * L - B rows are not touched.
 * out fp32 [B, C]; out_act (may be null) [B, ldo_act] in bf16, or fp32 when act_f32, columns [C, ldo_act) zero: the operand of the
 * projection GEMM; index_out (may be null) int32 [B], the chosen positions.  C a multiple of 8, at most 2048. */
enum { APTP_EOS_ARGMAX = 0, APTP_EOS_FIRST = 1 };
typedef struct {
  const int64_t* ids;
  const void* x; int64_t x_stride_b, x_stride_l;
  const float* gamma; const float* beta;
  float* out;
  void* out_act; int64_t ldo_act;
  int32_t* index_out;
  int32_t B, L, C;
  int32_t eos_mode, eos_token_id;
  int32_t x_f32, act_f32;
  float eps;
} AptpEosPoolLnParams;
int aptp_eos_pool_ln(const AptpEosPoolLnParams* p, aptp_stream_t stream);

/* cos_out[i] = a_i . b_i / (|a_i| |b_i|) for fp32 a, b [n, D] (clip_utils.py:159-166 without the normalised copies), one wave per
 * pair, and *sum_out = sum_i cos_out[i] in fp64 (accumulate: added to the value already there), summed by one workgroup in a fixed
 * order: bit-identical from run to run.  D a multiple of 4; lda, ldb multiples of 4. */
typedef struct {
  const float* a; int64_t lda;
  const float* b; int64_t ldb;
  float* cos_out;
  double* sum_out;
  int32_t n, D;
  int32_t accumulate;
} AptpPairedCosineParams;
int aptp_paired_cosine(const AptpPairedCosineParams* p, aptp_stream_t stream);

/* The training dataloader's transform (pdm/utils/data_utils.py:61-82) on a ragged batch of uint8 RGB images: Resize(R, BILINEAR)
 * on a PIL image, RandomCrop(R) or CenterCrop(R), RandomHorizontalFlip, ToTensor, Normalize(0.5, 0.5) -> pixel_values, NCHW
 * [B, 3, R, R] in fp32 (bf16 when out_f32 is 0):
 *   out[b, c, y, x] = (u / 255 - 0.5) / 0.5 in fp32,  u = resized_b[top + y, left + (flip ? R - 1 - x : x), c].
 * images: one flat uint8 buffer of images_bytes bytes, image b = [H, W, 3] at byte src_off.  The resize is PIL's 8-bit
 * ImagingResample as in aptp_image_patches_pil: the horizontal pass into a uint8 scratch image, then the vertical pass, each an
 * int32 accumulator that starts at 2^21, an arithmetic shift by 22 and a clamp to [0, 255].  The random draws are the caller's
 * (data.draw_crop_flip): the entry takes top, left and flip per image.
 *
 * tables: one int32 buffer of tables_count elements holding every coefficient table, built on the host (ops.pil_bilinear_table;
 * any filter in that format).  The table of an axis that goes from `in` to `out` samples with a window of k taps is, at its
 * element offset, bounds int32 [out, 2] = (first, count) followed by weights int32 [out, k] in 22-bit fixed point: out * (2 + k)
 * elements.  An axis whose size does not change takes no pass and has no table: its offset is APTP_TRAIN_NO_TABLE, the null
 * offset (an offset must be null exactly when the size does not change).  Images of equal sizes may share tables.
 *
 * Only what the crop window reads is computed.  The horizontal pass writes columns [left, left + R) of rows
 * [row0, row0 + nrows) of the source -- the rows the vertical windows of output rows [top, top + R) reach, from the caller's
 * vertical table; [top, top + R) itself when the height does not change -- into the image's scratch region, uint8 [nrows, R, 3]
 * at byte scratch_off (regions of different images must not overlap).  The second pass writes out.  Without a horizontal pass
 * scratch_off, row0 and nrows are not read.
 *
 * One descriptor row per image, 80 bytes, plain integers: */
#define APTP_TRAIN_NO_TABLE (-1)
typedef struct {
  int64_t src_off;             /* byte offset of the image in `images` */
  int64_t scratch_off;         /* byte offset of its region in `scratch` */
  int64_t xtab_off, ytab_off;  /* int32-element offsets of the horizontal / vertical table in `tables`, or APTP_TRAIN_NO_TABLE */
  int32_t H, W;                /* source extents */
  int32_t H1, W1;              /* resized extents */
  int32_t top, left, flip;     /* crop offsets in the resized image; flip 0 or 1 */
  int32_t xk, yk;              /* taps per row of the horizontal / vertical table */
  int32_t row0, nrows;         /* source rows the horizontal pass computes */
  int32_t reserved;            /* 0 */
} AptpTrainImageDesc;
/* desc is read on the HOST during the call and checked before anything is launched -- every offset and size against
 * images_bytes, tables_count and scratch_bytes, 0 <= top, top + R <= H1, 0 <= left, left + R <= W1, flip, the row range, R > 0,
 * B > 0 (at most 65535), null pointers: APTP_EINVAL and nothing launched.  desc_dev is the same B rows in device memory, which the
 * kernels read.  The kernels additionally clamp every window a table names to the rows and columns their pass owns, so no table
 * content can move a read outside its image or its scratch region.
 * At most two launches whatever the mix of sizes (the first only if some image's width changes), a 2-D grid: blockIdx.y is the
 * image, blockIdx.x a run of 256 pixels, workgroups past an image's own count exit at once. */
typedef struct {
  const uint8_t* images; int64_t images_bytes;
  const AptpTrainImageDesc* desc;          /* host */
  const AptpTrainImageDesc* desc_dev;      /* device */
  const int32_t* tables; int64_t tables_count;
  void* scratch; int64_t scratch_bytes;
  void* out;
  int32_t B, R;
  int32_t out_f32;
} AptpTrainImagesParams;
int aptp_train_images(const AptpTrainImagesParams* p, aptp_stream_t stream);

/* Everything a denoise step does after the U-Net call, in one launch: classifier-free guidance, the optional guidance
 * rescale, and the scheduler update (pipeline.py: PruningDenoiseLoop._one_step after the forward, DDIMSchedulerLite.step_coef,
 * PNDMSchedulerLite.step, DPMSolverMultistepSchedulerLite.step), in fp32, statement for statement.
 *   noise    the model output, contiguous [noise_rows, n], bf16 or fp32 (noise_dtype); with do_cfg noise_rows = 2 b laid out
 *            [uncond; text], without it noise_rows = b
 *   sample   fp32 [b, n];  out fp32 [b, n] (may be sample itself)
 *   g = u + guidance_scale (t - u)                                                       (do_cfg; otherwise g = noise)
 *   g <- phi g std(t) / std(g) + (1 - phi) g,  phi = guidance_rescale > 0                (needs do_cfg and n >= 2)
 *            std per sample over its n elements, unbiased (n - 1); summed in fp64 in a fixed order, no atomics
 * The scheduler state is DEVICE memory, read by the kernel, so a captured launch serves every step:
 *   DDIM     coef fp32 [4] = sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev), sqrt(1 - a_prev)
 *   PNDM     slot int64 [1], w fp32 [5], coef fp32 [2] = a_t, a_prev, flags fp32 [2] = use_saved, save, the ring E fp32
 *            [5, b, n] and saved fp32 [b, n]; E[slot] <- g and saved are updated in place (a slot outside 0..4 is clamped)
 *   DPMPP    DPM-Solver++ (2M): coef fp32 [5] = alpha_s, sigma_s, c_x, c_0, c_1 and, in saved, prev fp32 [b, n], the previous
 *            data prediction: x0 = alpha_s x - sigma_s g (v) or (x - sigma_s g) / alpha_s (epsilon),
 *            out = (c_x x + c_0 x0) + c_1 prev, prev <- x0 in place (zero-filled before the first call)
 * Without the rescale a flat grid over b n elements in groups of four (when every base is 16-byte aligned) plus single
 * elements; with it one workgroup per sample.  APTP_EINVAL and nothing launched for: null pointers, an unknown dtype /
 * scheduler / prediction type, noise_rows that is not b (2 b with do_cfg), misaligned pointers, guidance_rescale outside
 * [0, 1], a rescale without do_cfg or with n < 2, DPMPP without coef or prev. */
#define APTP_STEP_NOISE_BF16 0
#define APTP_STEP_NOISE_F32 1
#define APTP_STEP_DDIM 0
#define APTP_STEP_PNDM 1
#define APTP_STEP_DPMPP 2
#define APTP_STEP_EPSILON 0
#define APTP_STEP_V_PREDICTION 1
typedef struct {
  const void* noise;
  const float* sample;
  float* out;
  const float* coef;
  const int64_t* slot;
  const float* w;
  const float* flags;
  float* E;
  float* saved;
  int64_t n;
  int32_t b, noise_rows;
  int32_t noise_dtype, scheduler, prediction, do_cfg;
  float guidance_scale, guidance_rescale;
} AptpGuidedStepParams;
int aptp_guided_step(const AptpGuidedStepParams* p, aptp_stream_t stream);

/* Seeded normal noise (csrc/philox_normal.hip, the stream itself in csrc/philox_normal.h): Philox4x32-10 and Box-Muller in fp32,
 * every value a pure function of (seed of the sample, draw, element).  For sample r of b and element e of n:
 *   key (seeds_dev[r] & 0xffffffff, seeds_dev[r] >> 32) (the int64 read as uint64);  g = offset + e, blk = g >> 2, lane = g & 3;
 *   counter (blk & 0xffffffff, blk >> 32, d & 0xffffffff, d >> 32) with d = draw + draw_dev[0] (draw_dev may be null);
 *   z = lane `lane` of the block's four normals;  s = scale * scale_dev[0] (scale_dev may be null: s = scale)
 *   out[r, e] = s z,  or base[r, e] + s z with base (fp32 [b, n]; a multiply, then an add; out may be base)
 *   out is fp32, bf16 (the fp32 value rounded) or -- APTP_PHILOX_RAW -- the uint32 word x[lane] itself (no base, no scale_dev).
 * seeds_dev, draw_dev and scale_dev are DEVICE memory, read by the kernel, so a captured launch follows a loop.  A lane that owns
 * a whole aligned block of four does one Philox evaluation and one vector store; a row's head and tail, and everything when an
 * address is not aligned, go element by element with the same values.  APTP_EINVAL and nothing launched for: null out / seeds_dev,
 * an unknown out_kind, b outside 1..65535, n < 1, b n > 2^40, a negative offset or draw, misaligned pointers, raw with base or
 * scale_dev. */
#define APTP_PHILOX_F32 0
#define APTP_PHILOX_BF16 1
#define APTP_PHILOX_RAW 2
typedef struct {
  void* out;
  const float* base;
  const int64_t* seeds_dev;
  const int64_t* draw_dev;
  const float* scale_dev;
  int64_t n, offset, draw;
  int32_t b, out_kind;
  float scale;
} AptpPhiloxNormalParams;
int aptp_philox_normal(const AptpPhiloxNormalParams* p, aptp_stream_t stream);

/* A seeded training batch in one launch (csrc/train_noise.hip, the draw map and the arithmetic in csrc/train_noise.h): VAE moments
 * (or latents) and per-sample seeds -> noisy latents, target and timesteps, every value a pure function of (seed of the sample,
 * draw, element) on the stream of aptp_philox_normal.  With d = draw + draw_dev[0] (draw_dev may be null), sub-draw k is Philox
 * draw 8 d + k of seeds_dev[r]:  k = 1 posterior eps, 2 noise, 4 input perturbation (element e = c hw + y w + x of the sample's
 * [4, h, w]), 3 offset noise (element c), 5 timestep (word x0 of block 0: t = (x0 T) >> 32 in uint64); k = 0 is the host's crop
 * and flip.  In fp32, every product and sum rounded on its own, (sa, so) = sqrt_table[t]:
 *   x0     = scale fmaf(expf(0.5f clamp(logvar, -30, 20)), z1, mean)   (moments fp32 [B, 8, h, w], mean then logvar; the one
 *            fused multiply-add, as aptp_latent_dist's compiled statement has it: the same bits for the same eps)
 *          | latents_in                                            (fp32 [B, 4, h, w]);  exactly one of the two
 *   n      = z2 + noise_offset z3[c]         (z3 not drawn when noise_offset == 0)
 *   m      = n + input_perturbation z4       (z4 not drawn when input_perturbation == 0)
 *   noisy  = sa x0 + so m;   target = n (APTP_TRAIN_NOISE_EPSILON) | sa n - so x0 (APTP_TRAIN_NOISE_V_PREDICTION)
 * sqrt_table is fp32 [T, 2] = sqrt(alphas_cumprod), sqrt(1 - alphas_cumprod).  Outputs: noisy, target fp32 [B, 4, h, w],
 * timesteps int64 [B], optionally latents_out (x0) and noise_out (n).  seeds_dev and draw_dev are DEVICE memory, read by the
 * kernel, so a captured launch follows a device counter; the caller keeps d inside [0, 2^59).  A lane owns four elements of one
 * channel when h w % 4 == 0 and every tensor is 16-byte aligned, a single element otherwise, with the same bits.  APTP_EINVAL
 * and nothing launched (no host synchronisation) for: null required pointers, both or neither of moments and latents_in, B
 * outside 1..65535, h w < 1, T < 1, draw outside [0, 2^59), misaligned 4- or 8-byte pointers, an unknown prediction. */
#define APTP_TRAIN_NOISE_EPSILON 0
#define APTP_TRAIN_NOISE_V_PREDICTION 1
typedef struct {
  const float* moments;
  const float* latents_in;
  const float* sqrt_table;
  const int64_t* seeds_dev;
  const int64_t* draw_dev;
  float* noisy;
  float* target;
  int64_t* timesteps;
  float* latents_out;
  float* noise_out;
  int64_t draw;
  int32_t B, h, w, T;
  int32_t prediction;
  float scale, noise_offset, input_perturbation;
} AptpTrainNoiseParams;
int aptp_train_noise(const AptpTrainNoiseParams* p, aptp_stream_t stream);

const char* aptp_last_error(void);
int aptp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* APTP_HIP_H */
