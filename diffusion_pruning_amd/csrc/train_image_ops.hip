// The training dataloader's transform (pdm/utils/data_utils.py:61-82) on a ragged batch of uint8 images:
//   aptp_train_images   Resize(R, BILINEAR) on a PIL image -- PIL's 8-bit resampler, bit for bit -- a crop window, a horizontal
//                       flip, ToTensor and Normalize(0.5, 0.5), to NCHW pixel_values.  Two launches for the whole batch; only the
//                       columns and rows the crop window reads are resampled.
#include "aptp_common.h"

namespace {

// PIL's ImagingResample for 8-bit images (Resample.c), as in clip_score_ops.hip: PRECISION_BITS = 32 - 8 - 2
constexpr int PIL_BITS = 22;

__device__ __forceinline__ int pil_clip8(int acc) {
  const int v = acc >> PIL_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

struct TrainImgK {
  const uint8_t* images; const AptpTrainImageDesc* desc; const int32_t* tables;
  uint8_t* scratch; void* out;
  int R, out_f32;
};

// horizontal pass: blockIdx.y = image, one thread per pixel (r, x) of its scratch region [nrows, R, 3] -- source row row0 + r,
// column left + x of the resized width -- its three channels together
__global__ __launch_bounds__(256) void train_resample_h_kernel(const TrainImgK p) {
  const AptpTrainImageDesc d = p.desc[blockIdx.y];
  if (d.xtab_off < 0) return;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= d.nrows * p.R) return;
  const int r = idx / p.R, x = idx - r * p.R;
  const int ox = d.left + x;
  const int32_t* bounds = p.tables + d.xtab_off;
  const int32_t* k = bounds + 2 * (int64_t)d.W1 + (int64_t)ox * d.xk;
  int x0 = bounds[2 * ox], n = bounds[2 * ox + 1];
  // whatever the table says, the window stays inside the row
  x0 = x0 < 0 ? 0 : (x0 > d.W - 1 ? d.W - 1 : x0);
  n = n < 0 ? 0 : (n > d.xk ? d.xk : n);
  n = n > d.W - x0 ? d.W - x0 : n;
  const uint8_t* src = p.images + d.src_off + ((int64_t)(d.row0 + r) * d.W + x0) * 3;
  int a0 = 1 << (PIL_BITS - 1), a1 = a0, a2 = a0;
  for (int j = 0; j < n; ++j) {
    const int w = k[j];
    a0 += (int)src[3 * j] * w;
    a1 += (int)src[3 * j + 1] * w;
    a2 += (int)src[3 * j + 2] * w;
  }
  uint8_t* dst = p.scratch + d.scratch_off + (int64_t)idx * 3;
  dst[0] = (uint8_t)pil_clip8(a0);
  dst[1] = (uint8_t)pil_clip8(a1);
  dst[2] = (uint8_t)pil_clip8(a2);
}

// vertical pass + crop + flip + ToTensor + Normalize: blockIdx.y = image, one thread per output pixel (y, x), its three channel
// planes; consecutive lanes write consecutive x of one plane
__global__ __launch_bounds__(256) void train_pixels_kernel(const TrainImgK p) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.R * p.R) return;
  const AptpTrainImageDesc d = p.desc[blockIdx.y];
  const int y = idx / p.R, x = idx - y * p.R;
  const int cx = d.flip ? p.R - 1 - x : x;              // column of the crop window this output pixel shows
  // rows the pass may read: the scratch region holds source rows [row0, row0 + nrows) and the window's columns only
  const uint8_t* base;
  int64_t stride;
  int rbase, rcnt;
  if (d.xtab_off >= 0) {
    base = p.scratch + d.scratch_off + (int64_t)cx * 3;
    stride = (int64_t)p.R * 3; rbase = d.row0; rcnt = d.nrows;
  } else {
    base = p.images + d.src_off + (int64_t)(d.left + cx) * 3;
    stride = (int64_t)d.W * 3; rbase = 0; rcnt = d.H;
  }
  const int oy = d.top + y;
  int u0, u1, u2;
  if (d.ytab_off >= 0) {
    const int32_t* bounds = p.tables + d.ytab_off;
    const int32_t* w = bounds + 2 * (int64_t)d.H1 + (int64_t)oy * d.yk;
    int y0 = bounds[2 * oy], n = bounds[2 * oy + 1];
    y0 = y0 < rbase ? rbase : (y0 > rbase + rcnt - 1 ? rbase + rcnt - 1 : y0);
    n = n < 0 ? 0 : (n > d.yk ? d.yk : n);
    n = n > rbase + rcnt - y0 ? rbase + rcnt - y0 : n;
    const uint8_t* col = base + (int64_t)(y0 - rbase) * stride;
    int a0 = 1 << (PIL_BITS - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < n; ++j) {
      const int wj = w[j];
      a0 += (int)col[j * stride] * wj;
      a1 += (int)col[j * stride + 1] * wj;
      a2 += (int)col[j * stride + 2] * wj;
    }
    u0 = pil_clip8(a0); u1 = pil_clip8(a1); u2 = pil_clip8(a2);
  } else {
    int sy = oy < rbase ? rbase : (oy > rbase + rcnt - 1 ? rbase + rcnt - 1 : oy);
    const uint8_t* px = base + (int64_t)(sy - rbase) * stride;
    u0 = px[0]; u1 = px[1]; u2 = px[2];
  }
  // ToTensor (uint8 -> fp32, an IEEE division by 255) and Normalize ((v - 0.5) / 0.5), both in fp32 as torchvision does
  const float v0 = ((float)u0 / 255.0f - 0.5f) / 0.5f;
  const float v1 = ((float)u1 / 255.0f - 0.5f) / 0.5f;
  const float v2 = ((float)u2 / 255.0f - 0.5f) / 0.5f;
  const int64_t plane = (int64_t)p.R * p.R;
  const int64_t o = (int64_t)blockIdx.y * 3 * plane + idx;
  if (p.out_f32) {
    float* out = reinterpret_cast<float*>(p.out);
    out[o] = v0; out[o + plane] = v1; out[o + 2 * plane] = v2;
  } else {
    __bf16* out = reinterpret_cast<__bf16*>(p.out);
    out[o] = (__bf16)v0; out[o + plane] = (__bf16)v1; out[o + 2 * plane] = (__bf16)v2;
  }
}

constexpr int MAX_EXTENT = 65536;

}  // namespace

extern "C" int aptp_train_images(const AptpTrainImagesParams* p, aptp_stream_t stream) {
  APTP_CHECK(p && p->images && p->desc && p->desc_dev && p->out, "train_images: null pointer");
  APTP_CHECK(p->B > 0 && p->B <= 65535 && p->R > 0 && p->R <= 16384, "train_images: bad extents (B = %d in [1, 65535], R = %d in [1, 16384])", p->B, p->R);
  APTP_CHECK(p->images_bytes > 0 && p->tables_count >= 0 && p->scratch_bytes >= 0, "train_images: negative buffer size");
  APTP_CHECK(((uintptr_t)p->desc % 8) == 0 && ((uintptr_t)p->desc_dev % 8) == 0 && ((uintptr_t)p->tables % 4) == 0 &&
             ((uintptr_t)p->out % (p->out_f32 ? 4 : 2)) == 0, "train_images: pointer alignment");
  const int R = p->R;
  int max_hpix = 0;                                    // the longest horizontal pass of the batch, in pixels
  for (int b = 0; b < p->B; ++b) {
    const AptpTrainImageDesc& d = p->desc[b];
    APTP_CHECK(d.H > 0 && d.W > 0 && d.H1 > 0 && d.W1 > 0 && d.H <= MAX_EXTENT && d.W <= MAX_EXTENT && d.H1 <= MAX_EXTENT && d.W1 <= MAX_EXTENT,
               "train_images: image %d: extents %d x %d -> %d x %d must be in [1, %d]", b, d.H, d.W, d.H1, d.W1, MAX_EXTENT);
    APTP_CHECK(d.src_off >= 0 && d.src_off <= p->images_bytes && (int64_t)d.H * d.W * 3 <= p->images_bytes - d.src_off,
               "train_images: image %d: %d x %d x 3 bytes at offset %lld leave the image buffer of %lld bytes", b, d.H, d.W,
               (long long)d.src_off, (long long)p->images_bytes);
    APTP_CHECK(d.top >= 0 && d.left >= 0 && d.top <= d.H1 - R && d.left <= d.W1 - R,
               "train_images: image %d: the crop window (top %d, left %d, size %d) leaves the resized image %d x %d", b, d.top, d.left, R,
               d.H1, d.W1);
    APTP_CHECK(d.flip == 0 || d.flip == 1, "train_images: image %d: flip is %d (0 or 1)", b, d.flip);
    const bool horiz = d.xtab_off != APTP_TRAIN_NO_TABLE, vert = d.ytab_off != APTP_TRAIN_NO_TABLE;
    APTP_CHECK(horiz == (d.W1 != d.W) && vert == (d.H1 != d.H),
               "train_images: image %d: an axis has a table exactly when its size changes (%d x %d -> %d x %d)", b, d.H, d.W, d.H1, d.W1);
    if (horiz || vert) APTP_CHECK(p->tables, "train_images: image %d is resized: tables is needed", b);
    if (horiz) {
      APTP_CHECK(d.xk >= 1 && d.xk <= MAX_EXTENT && d.xtab_off >= 0 && d.xtab_off <= p->tables_count &&
                 (int64_t)d.W1 * (2 + d.xk) <= p->tables_count - d.xtab_off,
                 "train_images: image %d: the horizontal table (%d rows of 2 + %d at offset %lld) leaves the table buffer of %lld elements", b,
                 d.W1, d.xk, (long long)d.xtab_off, (long long)p->tables_count);
      APTP_CHECK(d.row0 >= 0 && d.nrows >= 1 && d.row0 <= d.H - d.nrows, "train_images: image %d: rows [%d, %d + %d) leave the image of %d rows", b,
                 d.row0, d.row0, d.nrows, d.H);
      APTP_CHECK(vert || (d.row0 <= d.top && d.top + R <= d.row0 + d.nrows),
                 "train_images: image %d: rows [%d, %d + %d) do not hold the crop window's rows [%d, %d + %d)", b, d.row0, d.row0, d.nrows, d.top,
                 d.top, R);
      APTP_CHECK(p->scratch, "train_images: image %d changes its width: scratch is needed", b);
      APTP_CHECK(d.scratch_off >= 0 && d.scratch_off <= p->scratch_bytes && (int64_t)d.nrows * R * 3 <= p->scratch_bytes - d.scratch_off,
                 "train_images: image %d: %d x %d x 3 scratch bytes at offset %lld leave the scratch buffer of %lld bytes", b, d.nrows, R,
                 (long long)d.scratch_off, (long long)p->scratch_bytes);
      APTP_CHECK((int64_t)d.nrows * R < (1ll << 31) - 256, "train_images: image %d: horizontal pass too large", b);
      if (d.nrows * R > max_hpix) max_hpix = d.nrows * R;
    }
    if (vert)
      APTP_CHECK(d.yk >= 1 && d.yk <= MAX_EXTENT && d.ytab_off >= 0 && d.ytab_off <= p->tables_count &&
                 (int64_t)d.H1 * (2 + d.yk) <= p->tables_count - d.ytab_off,
                 "train_images: image %d: the vertical table (%d rows of 2 + %d at offset %lld) leaves the table buffer of %lld elements", b,
                 d.H1, d.yk, (long long)d.ytab_off, (long long)p->tables_count);
  }
  TrainImgK k;
  k.images = p->images; k.desc = p->desc_dev; k.tables = p->tables; k.scratch = reinterpret_cast<uint8_t*>(p->scratch); k.out = p->out;
  k.R = R; k.out_f32 = p->out_f32 ? 1 : 0;
  if (max_hpix > 0) {
    hipLaunchKernelGGL(train_resample_h_kernel, dim3((unsigned)((max_hpix + 255) / 256), (unsigned)p->B), dim3(256), 0, (hipStream_t)stream, k);
    APTP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(train_pixels_kernel, dim3((unsigned)((R * R + 255) / 256), (unsigned)p->B), dim3(256), 0, (hipStream_t)stream, k);
  APTP_LAUNCH_CHECK();
  return APTP_OK;
}
