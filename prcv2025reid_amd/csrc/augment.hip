// Train / eval image transforms on the device (reference: datasets/dataset.py:284-307, train.py:1634-1641,
// tools/eval_mm_protocol.py:171-173), bit-exact against PIL + torch for given parameters:
//   Image.crop(box).resize((S, S), BILINEAR) -> mirror -> ImageEnhance.Brightness / .Contrast in the drawn order
//   -> ToTensor + Normalize (a host-built [3, 256] fp32 table) -> RandomErasing(value=0) on the erase box.
//
// Resize: PIL's ImagingResample, restated.  Separable, horizontal pass first; both passes round to uint8.  Per output sample
// the coefficients are those of precompute_coeffs (scale = in / out, support = max(scale, 1), triangle filter, normalised,
// all in double) converted to 22-bit fixed point with int(0.5 + w * 2^22); a pass accumulates 2^21 + sum v * k in int32 and
// keeps clamp(acc >> 22, 0, 255).  A pass whose size does not change has the coefficients [1, 0] and is an exact identity.
// Blend (Image.blend(degenerate, img, f)): trunc(float(d) + float(f) * float(v - d)) clamped to [0, 255]; d = 0 for brightness,
// d = int(mean luma + 0.5) for contrast, L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 over the image as it is at that point.
//
// Two launches per batch:
//   aug_resize_kernel  one workgroup per (image, band of R output rows, R * S <= 1024): the band's source rows pass through LDS
//                      CH rows at a time (horizontal pass -> uint8 LDS rows -> vertical taps accumulated in registers), so the
//                      LDS footprint is 10 976 B at S = 224 and the tap count (2 ceil(scale) + 1, any downscale) is a loop bound;
//                      a crop more than 100 times taller than wide that shrinks vertically takes the vertical pass first, as
//                      Image.resize does;
//                      brightness when it comes first; uint8 planar [n, 3, S, S] + the band's integer luma sum -> scratch
//   aug_finish_kernel  per (image, 4096 outputs): mean luma from the band sums, contrast (and brightness when second), flip,
//                      normalise through the table, erase, 16-byte fp32 stores
// Every source address is clamped into its own image (a malformed table entry cannot read outside it); an empty slot or an
// entry that does not fit the source buffer writes zeros.
#include "common.h"
#include <cstring>

// PIL computes its coefficients and blends without fused multiply-adds: so does this file
#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int CH = 8;                 // source rows per horizontal chunk
constexpr int MAX_SIDE = 8192;        // largest source height / width
constexpr int MAX_S = 1024;           // largest output side (S * S * 255 fits the int32 luma sum)
constexpr int FIELDS = 16;            // int32 per table entry (include/reid_hip.h)
constexpr int QPT = 4;                // float4 outputs per thread of the finishing pass
constexpr int TALL_W = MAX_SIDE / 100 + 1;   // widest crop that Image.resize takes vertical pass first (> 100 x taller)

struct AugParams {
    const uint8_t* src; long long src_bytes;
    const int32_t* table; const float* lut;
    uint8_t* mid;                     // [n, 3, S, S] resized (and brightened when brightness comes first) uint8
    int32_t* luma;                    // [n, nb] integer luma sum of each band
    float* out;                       // [n, 3, S, S]
    int n, S, R, nb;
};

struct Entry {
    long long off;
    int H, W, cx, cy, cw, ch, flags, ex, ey, ew, eh;
    float fb, fc;
    bool empty;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ Entry load_entry(const AugParams& p, int i) {
    const int32_t* t = p.table + (long long)i * FIELDS;
    Entry e;
    e.flags = t[8];
    e.off = (long long)(uint32_t)t[0] | ((long long)t[1] << 32);
    const int H = t[2], W = t[3];
    e.empty = (e.flags & REID_AUG_EMPTY) || H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE || e.off < 0 ||
              e.off > p.src_bytes - 3LL * H * W;
    e.H = clampi(H, 1, MAX_SIDE); e.W = clampi(W, 1, MAX_SIDE);
    e.cx = clampi(t[4], 0, e.W - 1); e.cy = clampi(t[5], 0, e.H - 1);
    e.cw = clampi(t[6], 1, e.W - e.cx); e.ch = clampi(t[7], 1, e.H - e.cy);
    e.fb = __int_as_float(t[9]); e.fc = __int_as_float(t[10]);
    e.ex = clampi(t[11], 0, p.S); e.ey = clampi(t[12], 0, p.S);
    e.ew = clampi(t[13], 0, p.S - e.ex); e.eh = clampi(t[14], 0, p.S - e.ey);
    return e;
}

__device__ __forceinline__ double tri(double x) {     // bilinear_filter of PIL's Resample.c
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

// One output sample of one pass (precompute_coeffs): first source index, tap count, centre and weight sum.
struct Axis { double center, ww; int lo, cnt; };

__device__ Axis axis_of(int in_size, double scale, double support, double ss, int o) {
    Axis a;
    a.center = (o + 0.5) * scale;
    int lo = (int)(a.center - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(a.center + support + 0.5);
    if (hi > in_size) hi = in_size;
    a.lo = lo; a.cnt = hi - lo;
    double ww = 0.0;
    for (int x = 0; x < a.cnt; ++x) ww += tri((x + lo - a.center + 0.5) * ss);     // PIL's summation order
    a.ww = ww;
    return a;
}

__device__ __forceinline__ int coeff(int src, double center, double ww, double ss) {   // normalize_coeffs_8bpc
    double k = tri((src - center + 0.5) * ss);
    if (ww != 0.0) k /= ww;
    return (int)(0.5 + k * 4194304.0);
}

__device__ __forceinline__ int clip8(int acc) { return clampi(acc >> 22, 0, 255); }

__device__ __forceinline__ int blend_u8(int d, int v, float f) {   // ImagingBlend; (int) truncates as PIL's (UINT8) cast does
    const float prod = f * (float)(v - d);
    return clampi((int)((float)d + prod), 0, 255);
}

__device__ __forceinline__ int luma_of(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

__device__ __forceinline__ int block_sum(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(NT) void aug_resize_kernel(const AugParams p) {
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    const int S = p.S, R = p.R, i = blockIdx.y, band = blockIdx.x, tid = threadIdx.x;
    const Entry e = load_entry(p, i);
    if (e.empty) return;                                     // (uniform: the finishing pass writes the zeros)
    double* col_c = (double*)dyn;                            // per output column: centre, weight sum, first tap, tap count
    double* col_w = col_c + S;
    double* row_c = col_w + S;                               // per output row of the band
    double* row_w = row_c + R;
    int* col_lo = (int*)(row_w + R);
    int* col_n = col_lo + S;
    int* row_lo = col_n + S;
    int* row_n = row_lo + R;
    int* kv = row_n + R;                                     // [R][CH] vertical coefficients of the current chunk
    uint8_t* tmp = (uint8_t*)(kv + R * CH);                  // [CH][S][3] horizontally resampled source rows ([R][cw][3]
                                                             // vertically resampled ones for a very tall crop)
    __shared__ int red[NT / 64];

    const int y0 = band * R, rows = min(R, S - y0);
    const double sx = (double)e.cw / S, sy = (double)e.ch / S;
    const double fx = sx < 1.0 ? 1.0 : sx, fy = sy < 1.0 ? 1.0 : sy;
    const double ssx = 1.0 / fx, ssy = 1.0 / fy;
    for (int xx = tid; xx < S; xx += NT) {
        const Axis a = axis_of(e.cw, sx, fx, ssx, xx);
        col_c[xx] = a.center; col_w[xx] = a.ww; col_lo[xx] = a.lo; col_n[xx] = a.cnt;
    }
    if (tid < rows) {
        const Axis a = axis_of(e.ch, sy, fy, ssy, y0 + tid);
        row_c[tid] = a.center; row_w[tid] = a.ww; row_lo[tid] = a.lo; row_n[tid] = a.cnt;
    }
    __syncthreads();

    const uint8_t* img = p.src + e.off;
    const long long pitch = 3LL * e.W;
    int v[4][3];
    if (e.ch > 100 * e.cw && S < e.ch) {
        // Image.resize takes a crop more than 100 times taller than wide that shrinks vertically in two calls, vertical pass
        // first: the band's rows of the vertically resampled crop (cw <= 81 columns) -> LDS -> horizontal taps
        for (int t = tid; t < rows * e.cw; t += NT) {
            const int r = t / e.cw, x = t - r * e.cw;
            int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
            const uint8_t* s = img + (long long)(e.cy + row_lo[r]) * pitch + 3LL * (e.cx + x);
            for (int j = 0; j < row_n[r]; ++j) {
                const int k = coeff(row_lo[r] + j, row_c[r], row_w[r], ssy);
                const uint8_t* q = s + j * pitch;
                a0 += q[0] * k; a1 += q[1] * k; a2 += q[2] * k;
            }
            tmp[3 * t] = (uint8_t)clip8(a0); tmp[3 * t + 1] = (uint8_t)clip8(a1); tmp[3 * t + 2] = (uint8_t)clip8(a2);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q = tid + k * NT;
            if (q < rows * S) {
                const int r = q / S, xx = q - r * S, lo = col_lo[xx];
                int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
                for (int x = 0; x < col_n[xx]; ++x) {
                    const int kk = coeff(lo + x, col_c[xx], col_w[xx], ssx);
                    const uint8_t* s = tmp + 3 * (r * e.cw + lo + x);
                    a0 += s[0] * kk; a1 += s[1] * kk; a2 += s[2] * kk;
                }
                v[k][0] = clip8(a0); v[k][1] = clip8(a1); v[k][2] = clip8(a2);
            }
        }
    } else {
        int acc[4][3];
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 1 << 21;
        const int ya1 = row_lo[rows - 1] + row_n[rows - 1];
        for (int ya = row_lo[0]; ya < ya1; ya += CH) {
            const int nr = min(CH, ya1 - ya);
            // horizontal pass of source rows [ya, ya + nr) of the crop: one output column per thread, all nr rows per tap
            for (int xx = tid; xx < S; xx += NT) {
                const double c = col_c[xx], w = col_w[xx];
                const int lo = col_lo[xx], cnt = col_n[xx];
                int h[CH][3];
#pragma unroll
                for (int j = 0; j < CH; ++j) h[j][0] = h[j][1] = h[j][2] = 1 << 21;
                const uint8_t* base = img + (long long)(e.cy + ya) * pitch + 3LL * (e.cx + lo);
                for (int x = 0; x < cnt; ++x) {
                    const int k = coeff(x + lo, c, w, ssx);
                    const uint8_t* s = base + 3 * x;
#pragma unroll
                    for (int j = 0; j < CH; ++j)
                        if (j < nr) {
                            const uint8_t* q = s + j * pitch;
                            h[j][0] += q[0] * k; h[j][1] += q[1] * k; h[j][2] += q[2] * k;
                        }
                }
#pragma unroll
                for (int j = 0; j < CH; ++j)
                    if (j < nr) {
                        uint8_t* d = tmp + 3 * (j * S + xx);
                        d[0] = (uint8_t)clip8(h[j][0]); d[1] = (uint8_t)clip8(h[j][1]); d[2] = (uint8_t)clip8(h[j][2]);
                    }
            }
            for (int t = tid; t < rows * CH; t += NT) {
                const int r = t / CH, y = ya + t % CH;
                kv[t] = (t % CH < nr && y >= row_lo[r] && y < row_lo[r] + row_n[r]) ? coeff(y, row_c[r], row_w[r], ssy) : 0;
            }
            __syncthreads();
            // vertical taps of this chunk for the band's output pixels (up to 4 per thread)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int q = tid + k * NT;
                if (q < rows * S) {
                    const int r = q / S, xx = q - r * S;
                    for (int j = 0; j < nr; ++j) {
                        const int kk = kv[r * CH + j];
                        const uint8_t* s = tmp + 3 * (j * S + xx);
                        acc[k][0] += s[0] * kk; acc[k][1] += s[1] * kk; acc[k][2] += s[2] * kk;
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) v[k][c] = clip8(acc[k][c]);
    }

    const bool bright_first = !(e.flags & REID_AUG_CONTRAST_FIRST);
    int lsum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int q = tid + k * NT;
        if (q < rows * S) {
            const int r = q / S, xx = q - r * S;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (bright_first) v[k][c] = blend_u8(0, v[k][c], e.fb);
                p.mid[(((long long)i * 3 + c) * S + y0 + r) * S + xx] = (uint8_t)v[k][c];
            }
            lsum += luma_of(v[k][0], v[k][1], v[k][2]);
        }
    }
    lsum = block_sum(lsum, red);
    if (tid == 0) p.luma[(long long)i * p.nb + band] = lsum;
}

__global__ __launch_bounds__(NT) void aug_finish_kernel(const AugParams p) {
    __shared__ float lut[3 * 256];
    __shared__ int red[NT / 64];
    const int S = p.S, i = blockIdx.y, tid = threadIdx.x;
    const Entry e = load_entry(p, i);
    const int qrow = S / 4, qplane = S * qrow, quads = 3 * qplane;
    f32x4* out = (f32x4*)(p.out + (long long)i * 3 * S * S);
    const int q0 = blockIdx.x * NT * QPT + tid;
    if (e.empty) {
#pragma unroll
        for (int k = 0; k < QPT; ++k)
            if (q0 + k * NT < quads) out[q0 + k * NT] = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    for (int t = tid; t < 3 * 256; t += NT) lut[t] = p.lut[t];
    int d = 0;
    if (e.fc != 1.0f) {                                      // (uniform) contrast: PIL's int(mean + 0.5) of the luma
        int s = 0;
        for (int t = tid; t < p.nb; t += NT) s += p.luma[(long long)i * p.nb + t];
        s = block_sum(s, red);
        d = (int)((double)s / ((double)S * S) + 0.5);
    }
    __syncthreads();
    const bool contrast_first = e.flags & REID_AUG_CONTRAST_FIRST, flip = e.flags & REID_AUG_FLIP;
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
        const int q = q0 + k * NT;
        if (q >= quads) break;
        const int c = q / qplane, rem = q - c * qplane, y = rem / qrow, x = 4 * (rem - y * qrow);
        const uint32_t word = *(const uint32_t*)(p.mid + (((long long)i * 3 + c) * S + y) * S + (flip ? S - 4 - x : x));
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int v = (word >> (8 * (flip ? 3 - j : j))) & 255;
            v = blend_u8(d, v, e.fc);
            if (contrast_first) v = blend_u8(0, v, e.fb);
            const bool erased = y >= e.ey && y < e.ey + e.eh && x + j >= e.ex && x + j < e.ex + e.ew;
            o[j] = erased ? 0.f : lut[c * 256 + v];
        }
        out[q] = f32x4{o[0], o[1], o[2], o[3]};
    }
}

}  // namespace

extern "C" int64_t reid_augment_ws_bytes(int32_t n, int32_t S) {
    if (n < 1 || S < 4 || S > MAX_S) return 0;
    const int R = min(4, MAX_S / S), nb = (S + R - 1) / R;
    return (3LL * n * S * S + 255) / 256 * 256 + 4LL * n * nb;
}

extern "C" int reid_augment_images(const void* src, int64_t src_bytes, const int32_t* table, const int32_t* host_table, int32_t n,
                                   int32_t S, const float* lut, void* ws, int64_t ws_bytes, float* out, void* stream) {
    REID_CHECK_ARG(src && table && host_table && lut && ws && out, "reid_augment_images: null pointer");
    REID_CHECK_ARG(n >= 1 && n <= 65535, "reid_augment_images: n=%d (1..65535)", n);
    REID_CHECK_ARG(S >= 4 && S <= MAX_S && S % 4 == 0, "reid_augment_images: S=%d (4..%d, S %% 4 == 0)", S, MAX_S);
    REID_CHECK_ARG(((uintptr_t)out & 15) == 0 && ((uintptr_t)ws & 15) == 0, "reid_augment_images: out and ws must be 16-byte aligned");
    REID_CHECK_ARG(ws_bytes >= reid_augment_ws_bytes(n, S), "reid_augment_images: ws_bytes=%lld < %lld", (long long)ws_bytes,
                   (long long)reid_augment_ws_bytes(n, S));
    for (int i = 0; i < n; ++i) {
        const int32_t* t = host_table + (int64_t)i * FIELDS;
        const int flags = t[8];
        REID_CHECK_ARG((flags & ~(REID_AUG_FLIP | REID_AUG_CONTRAST_FIRST | REID_AUG_EMPTY)) == 0, "reid_augment_images: image %d: flags=%d", i, flags);
        if (flags & REID_AUG_EMPTY) continue;
        const int64_t off = (int64_t)(uint32_t)t[0] | ((int64_t)t[1] << 32);
        const int H = t[2], W = t[3], cx = t[4], cy = t[5], cw = t[6], ch = t[7];
        REID_CHECK_ARG(H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "reid_augment_images: image %d: %d x %d (1..%d)", i, H, W, MAX_SIDE);
        REID_CHECK_ARG(off >= 0 && off + 3LL * H * W <= src_bytes, "reid_augment_images: image %d: bytes [%lld, %lld) outside src_bytes=%lld",
                       i, (long long)off, (long long)(off + 3LL * H * W), (long long)src_bytes);
        REID_CHECK_ARG(cx >= 0 && cy >= 0 && cw >= 1 && ch >= 1 && cx + cw <= W && cy + ch <= H,
                       "reid_augment_images: image %d: crop (%d, %d, %d, %d) outside %d x %d", i, cx, cy, cw, ch, H, W);
        float fb, fc;
        std::memcpy(&fb, &t[9], 4); std::memcpy(&fc, &t[10], 4);
        REID_CHECK_ARG(fb >= 0.f && fb <= 1e6f && fc >= 0.f && fc <= 1e6f, "reid_augment_images: image %d: jitter factors %g %g", i, fb, fc);
        REID_CHECK_ARG(t[11] >= 0 && t[12] >= 0 && t[13] >= 0 && t[14] >= 0 && t[11] + t[13] <= S && t[12] + t[14] <= S,
                       "reid_augment_images: image %d: erase box (%d, %d, %d, %d) outside %d x %d", i, t[11], t[12], t[13], t[14], S, S);
    }
    const int R = min(4, MAX_S / S), nb = (S + R - 1) / R;
    AugParams p{(const uint8_t*)src, (long long)src_bytes, table, lut, (uint8_t*)ws,
                (int32_t*)((char*)ws + (3LL * n * S * S + 255) / 256 * 256), out, n, S, R, nb};
    const size_t lds = (size_t)(2 * S + 2 * R) * 8 + (size_t)(2 * S + 2 * R + R * CH) * 4 + (size_t)max(CH * S, R * TALL_W) * 3;
    hipLaunchKernelGGL(aug_resize_kernel, dim3(nb, n), dim3(NT), lds, (hipStream_t)stream, p);
    REID_CHECK_LAUNCH("reid_augment_images: resize");
    const int quads = 3 * S * S / 4;
    hipLaunchKernelGGL(aug_finish_kernel, dim3((quads + NT * QPT - 1) / (NT * QPT), n), dim3(NT), 0, (hipStream_t)stream, p);
    REID_CHECK_LAUNCH("reid_augment_images: finish");
    return REID_OK;
}
