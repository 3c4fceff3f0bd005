// Training-sample preparation on the device (gfx950): what KittiLoader.__getitem__ does per sample on the host besides the point-cloud
// down-sampling of scan_prep.hip.
//
// Replaces  data/kitti_pc_img_pose_loader.py:326-349  top-row crop, x0.5 resize, crop window, the matching K updates (kitti_helper.py:193-203)
//           :120-134                                  torchvision ColorJitter on a PIL image (brightness, contrast, saturation, hue; shuffled)
//           :136-156, :352-384                        the random pose Pr, the mirror flip, Pr . P_cam_nwu and the ground-truth P
//           :199-232                                  the per-scan rigid transform of multi-scan accumulation
//           :439                                      uint8 HWC -> float32 CHW
// (the Gaussian jitter :108-118 is fused into scan_prep.hip's ragged gather.)
//
// Draws: Philox stream tag 4, counter (frame, block k, 0, 4), two 53-bit uniforms per block -- a pure function of (seed, frame).
// Colour arithmetic is PIL's, value for value (tests pin it against PIL): Image.blend in float32 with a separately rounded multiply and
// add (this file is built with FMA contraction off, and the blend spells the roundings out), clip, truncate; RGB <-> HSV as Convert.c does.
// The resize is the rounded 2x2 mean, which is what OpenCV's INTER_LINEAR gives at an exact factor of two (restated, not pinned).
//
// Oxford / nuScenes loaders (data/oxford_pc_img_pose_loader.py:220-380, data/nuscenes_pc_img_pose_loader.py:273-408; the _ds entry points):
// the same kernels with a bottom-row crop, the centre-pick resize 1/k for odd k (with an explicit dsize OpenCV's scale is src / dst = k exactly,
// the sample coordinate (d + 0.5) k - 0.5 is the integer k d + (k - 1) / 2, the bilinear weights are exactly (1, 0) and the fixed-point path
// returns the pixel itself -- derived, not checked against OpenCV), a per-frame colour enable (one further uniform, block 7), no flip,
// Pr applied in the frame the cloud is stored in, P = P_cam_pc . Pr^-1, and val_random_Ry about the data set's axis.
#include "common.h"
#include "philox.h"

namespace {

enum { OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2, OP_HUE = 3 };
enum { I_DX = 0, I_DY = 1, I_FLIP = 2, I_OP0 = 3, I_HUE_SHIFT = 7, INTS = 8 };
enum { DS_KITTI = 0, DS_OXFORD = 1, DS_NUSCENES = 2 };

__constant__ unsigned char kPerms[24][4] = {{0, 1, 2, 3}, {0, 1, 3, 2}, {0, 2, 1, 3}, {0, 2, 3, 1}, {0, 3, 1, 2}, {0, 3, 2, 1}, {1, 0, 2, 3}, {1, 0, 3, 2},
                                            {1, 2, 0, 3}, {1, 2, 3, 0}, {1, 3, 0, 2}, {1, 3, 2, 0}, {2, 0, 1, 3}, {2, 0, 3, 1}, {2, 1, 0, 3}, {2, 1, 3, 0},
                                            {2, 3, 0, 1}, {2, 3, 1, 0}, {3, 0, 1, 2}, {3, 0, 2, 1}, {3, 1, 0, 2}, {3, 1, 2, 0}, {3, 2, 0, 1}, {3, 2, 1, 0}};

__device__ void matmul4(const double* A, const double* Bm, double* C) {      // C = A . B, each sum in ascending k
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            double s = A[4 * r] * Bm[c];
            for (int k = 1; k < 4; ++k) s = s + A[4 * r + k] * Bm[4 * k + c];
            C[4 * r + c] = s;
        }
}

// ---------------------------------------------------------------- a. per-frame draws and small matrices: one thread per frame
__global__ __launch_bounds__(64) void sample_draws_kernel(unsigned long long seed, const unsigned long long* __restrict__ seed_dev, int B, int frame0,
                                                          di2p_sample_opt_t o, const double* __restrict__ K, const double* __restrict__ Pc,
                                                          const double* __restrict__ Pji, int* __restrict__ ints, float* __restrict__ factors,
                                                          double* __restrict__ Pr_out, double* __restrict__ PrPcn_out, float* __restrict__ P_out,
                                                          float* __restrict__ K_out, int dataset, int* __restrict__ enable,
                                                          float* __restrict__ t_ij) {
    // dataset DS_KITTI: di2p_sample_draws.  DS_OXFORD / DS_NUSCENES (di2p_sample_draws_ds): the same uniforms for the same items, no flip, the
    // colour enable from u[14] (block 7, which KITTI frames never draw), Pc is P_cam_pc and the cloud stays in the frame it is stored in
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= B) return;
    if (seed_dev) seed = *seed_dev;
    double u[16];
    for (int k = 0; k < (dataset == DS_KITTI ? 7 : 8); ++k) {
        const U4 r = philox4x32_10(U4{(unsigned)(frame0 + j), (unsigned)k, 0u, 4u}, (unsigned)seed, (unsigned)(seed >> 32));
        u[2 * k] = u53(r.x, r.y);
        u[2 * k + 1] = u53(r.z, r.w);
    }
    int dx, dy, flip = 0, perm = 0;
    double f[4] = {1.0, 1.0, 1.0, 0.0}, t[3] = {0.0, 0.0, 0.0}, ang[3] = {0.0, 0.0, 0.0};
    if (o.mode == 0) {
        const int nx = o.Ws - o.img_W + 1, ny = o.Hs - o.img_H + 1;
        dx = min((int)(u[0] * nx), nx - 1);
        dy = min((int)(u[1] * ny), ny - 1);
        flip = dataset == DS_KITTI && u[2] > 0.5 ? 1 : 0;
        perm = min((int)(u[3] * 24), 23);
        for (int k = 0; k < 4; ++k) f[k] = o.color_range[2 * k] + (o.color_range[2 * k + 1] - o.color_range[2 * k]) * u[4 + k];
        for (int k = 0; k < 3; ++k) t[k] = o.amplitude[k] * (2.0 * u[8 + k] - 1.0);
        for (int k = 0; k < 3; ++k) ang[k] = o.amplitude[3 + k] * (2.0 * u[11 + k] - 1.0);
    } else {
        dx = (o.Ws - o.img_W) / 2;
        dy = (o.Hs - o.img_H) / 2;
        // val_random_Ry: generate_random_transform(0, 0, 0, 0, 2 pi, 0) -- the amplitude is fixed, P_Ry_amplitude is not read (:367-368);
        // the angle comes from u[12], the uniform that is the Ry draw in train mode too
        // (:302-304 Oxford: about y as KITTI; nuScenes :339-341: about z, from u[13], the Rz draw of train mode)
        const int axis = dataset == DS_NUSCENES ? 2 : 1;
        if (o.mode == 2) ang[axis] = (2.0 * 3.141592653589793) * (2.0 * u[11 + axis] - 1.0);
    }
    int* I = ints + INTS * (long long)j;
    I[I_DX] = dx; I[I_DY] = dy; I[I_FLIP] = flip;
    for (int k = 0; k < 4; ++k) I[I_OP0 + k] = kPerms[perm][k];
    I[I_HUE_SHIFT] = (int)(f[3] * 255.0) & 255;          // np.uint8(hue_factor * 255): truncation, then wrap-around
    for (int k = 0; k < 4; ++k) factors[4 * (long long)j + k] = (float)f[k];
    if (enable) enable[j] = o.mode == 0 && u[14] > 0.5 ? 1 : 0;          // if random.random() > 0.5: augment_img

    // Pr = [Rz Ry Rx | t] (augmentation.angles2rotation_matrix), times diag(-1, 1, 1, 1) when flipped
    const double cx = cos(ang[0]), sx = sin(ang[0]), cy = cos(ang[1]), sy = sin(ang[1]), cz = cos(ang[2]), sz = sin(ang[2]);
    const double Rx[16] = {1, 0, 0, 0, 0, cx, -sx, 0, 0, sx, cx, 0, 0, 0, 0, 1}, Ry[16] = {cy, 0, sy, 0, 0, 1, 0, 0, -sy, 0, cy, 0, 0, 0, 0, 1},
                 Rz[16] = {cz, -sz, 0, 0, sz, cz, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    double Ryx[16], Pr[16];
    matmul4(Ry, Rx, Ryx);
    matmul4(Rz, Ryx, Pr);
    for (int r = 0; r < 3; ++r) {
        Pr[4 * r + 3] = t[r];
        if (flip) Pr[4 * r] = -Pr[4 * r];
    }
    const double Pcn[16] = {0, -1, 0, 0, 0, 0, -1, 0, 1, 0, 0, 0, 0, 0, 0, 1}, Pnc[16] = {0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 0, 1};
    double Pinv[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, A[16], Bm[16], C[16];
    for (int r = 0; r < 3; ++r) {          // rigid inverse in closed form: [R^T | -R^T t]
        for (int c = 0; c < 3; ++c) Pinv[4 * r + c] = Pr[4 * c + r];
        Pinv[4 * r + 3] = -((Pr[r] * t[0] + Pr[4 + r] * t[1]) + Pr[8 + r] * t[2]);
    }
    if (dataset == DS_KITTI) {
        matmul4(Pr, Pcn, A);
        for (int k = 0; k < 16; ++k) {
            Pr_out[16 * (long long)j + k] = Pr[k];
            PrPcn_out[16 * (long long)j + k] = A[k];
        }
        matmul4(Pnc, Pinv, A);
        matmul4(Pc + 16 * (long long)j, A, Bm);
        if (Pji) matmul4(Pji + 16 * (long long)j, Bm, C);
        for (int k = 0; k < 12; ++k) P_out[12 * (long long)j + k] = (float)(Pji ? C[k] : Bm[k]);
    } else {          // the point kernels' transform is Pr itself; P = P_cam_pc . Pr^-1, t_ij = P_cam_pc[:3, 3]
        for (int k = 0; k < 16; ++k) Pr_out[16 * (long long)j + k] = Pr[k];
        matmul4(Pc + 16 * (long long)j, Pinv, Bm);
        for (int k = 0; k < 12; ++k) P_out[12 * (long long)j + k] = (float)Bm[k];
        if (t_ij) for (int r = 0; r < 3; ++r) t_ij[3 * (long long)j + r] = (float)Pc[16 * (long long)j + 4 * r + 3];
    }

    // K': crop the top rows, scale (K[2][2] back to 1), crop the window.  The flip does not touch K (neither does the reference), and
    // neither does Oxford's bottom-row crop (its crop_top is 0: K - 0.0 is K).
    double Kc[9];
    for (int k = 0; k < 9; ++k) Kc[k] = K[9 * (long long)j + k];
    Kc[5] -= (double)o.crop_top;
    for (int k = 0; k < 9; ++k) Kc[k] = o.img_scale * Kc[k];
    Kc[8] = 1.0;
    Kc[2] -= (double)dx;
    Kc[5] -= (double)dy;
    for (int k = 0; k < 9; ++k) K_out[9 * (long long)j + k] = (float)Kc[k];
}

// ---------------------------------------------------------------- b. image path
struct ImgGeom { int H0, W0, top, half, H, W, max_dx, max_dy, k, noflip; };          // k: centre pick of k x k (1: the pixel itself)

struct FrameDraw { int dx, dy, flip, op[4], shift; float f[3]; int color; };

__device__ __forceinline__ FrameDraw load_draw(const int* __restrict__ ints, const float* __restrict__ factors, const int* __restrict__ enable, int b,
                                               const ImgGeom& g, int geometry) {
    FrameDraw d{0, 0, 0, {0, 1, 2, 3}, 0, {1.0f, 1.0f, 1.0f}, 1};
    if (!ints || !factors) return d;      // neither geometry nor colour: plain uint8 HWC -> float32 CHW
    const int* I = ints + INTS * (long long)b;
    // clamped: a caller-supplied table can never move the window outside the image
    d.dx = geometry ? min(max(I[I_DX], 0), g.max_dx) : 0;
    d.dy = geometry ? min(max(I[I_DY], 0), g.max_dy) : 0;
    d.flip = geometry && !g.noflip ? (I[I_FLIP] & 1) : 0;
    d.color = enable ? (enable[b] != 0) : 1;
    for (int k = 0; k < 4; ++k) d.op[k] = I[I_OP0 + k] & 3;
    d.shift = I[I_HUE_SHIFT] & 255;
    for (int k = 0; k < 3; ++k) d.f[k] = factors[4 * (long long)b + k];
    return d;
}

// pixel (y, x) of the crop window before the flip: the rounded 2x2 mean of the source (scale 0.5), the source pixel (scale 1) or the centre
// pixel of the k x k block (scale 1 / k, k odd)
__device__ __forceinline__ void fetch(const unsigned char* __restrict__ img, const ImgGeom& g, const FrameDraw& d, int y, int x, int c[3]) {
    const int sy = d.dy + y, sx = d.dx + x;
    if (g.half) {
        const unsigned char* r0 = img + ((long long)(g.top + 2 * sy) * g.W0 + 2 * sx) * 3;
        const unsigned char* r1 = r0 + (long long)g.W0 * 3;
        for (int k = 0; k < 3; ++k) c[k] = ((int)r0[k] + (int)r0[3 + k] + (int)r1[k] + (int)r1[3 + k] + 2) >> 2;
    } else {
        const int h = (g.k - 1) >> 1;
        const unsigned char* r0 = img + ((long long)(g.top + g.k * sy + h) * g.W0 + g.k * sx + h) * 3;
        for (int k = 0; k < 3; ++k) c[k] = r0[k];
    }
}

__device__ __forceinline__ int grey_of(const int c[3]) { return (19595 * c[0] + 38470 * c[1] + 7471 * c[2] + 0x8000) >> 16; }

// Image.blend(degenerate, image, factor): t = d + f * (p - d), multiply and add rounded separately; t <= 0 -> 0, t >= 255 -> 255, else truncation
__device__ __forceinline__ int blend(int d, int p, float f) {
    const float t = __fadd_rn((float)d, __fmul_rn(f, (float)(p - d)));
    return t <= 0.0f ? 0 : t >= 255.0f ? 255 : (int)t;
}

// adjust_hue: PIL's rgb2hsv, H += shift (mod 256), PIL's hsv2rgb (Convert.c: uint8 channels, float intermediates where C keeps a float,
// double where C promotes, truncation into H and S, round-half-away into R, G, B)
__device__ void hue_op(int c[3], int shift) {
    const int r = c[0], g = c[1], b = c[2];
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    int uh = 0, us = 0;
    const int v = maxc;
    if (minc != maxc) {
        const float cr = (float)(maxc - minc);
        const float s = __fdiv_rn(cr, (float)maxc);
        const float rc = __fdiv_rn((float)(maxc - r), cr), gc = __fdiv_rn((float)(maxc - g), cr), bc = __fdiv_rn((float)(maxc - b), cr);
        float h;
        if (r == maxc) h = __fsub_rn(bc, gc);
        else if (g == maxc) h = (float)((2.0 + (double)rc) - (double)bc);
        else h = (float)((4.0 + (double)gc) - (double)rc);
        double hh = (double)h / 6.0 + 1.0;          // in [5/6, 11/6]: fmod(hh, 1.0)
        if (hh >= 1.0) hh -= 1.0;
        h = (float)hh;
        uh = min(max((int)((double)h * 255.0), 0), 255);
        us = min(max((int)((double)s * 255.0), 0), 255);
    }
    uh = (uh + shift) & 255;
    if (us == 0) {
        c[0] = c[1] = c[2] = v;
        return;
    }
    const double h6 = (double)(float)uh * 6.0 / 255.0;
    const double fi = floor(h6);
    const double f = (double)(float)(h6 - fi);
    const double fs = (double)(float)((double)(float)us / 255.0);
    const double vd = (double)(float)v;
    const int p = min(max((int)round(vd * (1.0 - fs)), 0), 255);
    const int q = min(max((int)round(vd * (1.0 - fs * f)), 0), 255);
    const int t = min(max((int)round(vd * (1.0 - fs * (1.0 - f))), 0), 255);
    switch ((int)fi % 6) {
        case 0: c[0] = v; c[1] = t; c[2] = p; break;
        case 1: c[0] = q; c[1] = v; c[2] = p; break;
        case 2: c[0] = p; c[1] = v; c[2] = t; break;
        case 3: c[0] = p; c[1] = q; c[2] = v; break;
        case 4: c[0] = t; c[1] = p; c[2] = v; break;
        default: c[0] = v; c[1] = p; c[2] = q; break;
    }
}

__device__ __forceinline__ void color_op(int op, int c[3], const FrameDraw& d, int mean) {
    if (op == OP_HUE) {
        hue_op(c, d.shift);
        return;
    }
    const int L = op == OP_SATURATION ? grey_of(c) : op == OP_CONTRAST ? mean : 0;
    for (int k = 0; k < 3; ++k) c[k] = blend(L, c[k], d.f[op]);
}

__global__ __launch_bounds__(256) void zero_sums_kernel(unsigned* __restrict__ sums, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) sums[b] = 0u;
}

// launch 1: sums[b] = sum over the window of the grey level after the operations that precede the contrast operation in this frame's order.
// An integer sum (160 * 512 * 255 < 2^32), so it does not depend on the grid.
__global__ __launch_bounds__(256) void grey_sum_kernel(const unsigned char* __restrict__ images, ImgGeom g, const int* __restrict__ ints,
                                                       const float* __restrict__ factors, const int* __restrict__ enable, int geometry,
                                                       unsigned* __restrict__ sums) {
    __shared__ unsigned part[4];
    const int b = blockIdx.y;
    const FrameDraw d = load_draw(ints, factors, enable, b, g, geometry);
    if (!d.color) return;          // uniform over the workgroup: a frame without colour needs no sum
    const unsigned char* img = images + (long long)b * g.H0 * g.W0 * 3;
    unsigned acc = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < g.H * g.W; i += gridDim.x * 256) {
        int c[3];
        fetch(img, g, d, i / g.W, i % g.W, c);
        for (int k = 0; k < 4 && d.op[k] != OP_CONTRAST; ++k) color_op(d.op[k], c, d, 0);
        acc += (unsigned)grey_of(c);
    }
    for (int s = 32; s > 0; s >>= 1) acc += __shfl_down(acc, s, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sums + b, part[0] + part[1] + part[2] + part[3]);
}

// launch 2: 2x2 box -> colour chain in this frame's order -> flip -> three coalesced float32 plane stores
__global__ __launch_bounds__(256) void image_apply_kernel(const unsigned char* __restrict__ images, ImgGeom g, const int* __restrict__ ints,
                                                          const float* __restrict__ factors, const int* __restrict__ enable, int geometry,
                                                          int color, const unsigned* __restrict__ sums, float* __restrict__ out) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.H * g.W) return;
    const FrameDraw d = load_draw(ints, factors, enable, b, g, geometry);
    const int y = i / g.W, x = i % g.W;
    int c[3];
    fetch(images + (long long)b * g.H0 * g.W0 * 3, g, d, y, d.flip ? g.W - 1 - x : x, c);
    if (color && d.color) {
        const unsigned long long n = (unsigned long long)g.H * g.W;
        const int mean = (int)((2ull * sums[b] + n) / (2ull * n));          // int(sum / count + 0.5), exactly
        for (int k = 0; k < 4; ++k) color_op(d.op[k], c, d, mean);
    }
    float* o = out + (long long)b * 3 * g.H * g.W + i;
    for (int k = 0; k < 3; ++k) o[(long long)k * g.H * g.W] = (float)c[k];
}

// ---------------------------------------------------------------- d. accumulation: one rigid transform per segment
__global__ __launch_bounds__(256) void transform_segments_kernel(const float* pts, const float* nrm, const int* __restrict__ seg,
                                                                 const double* __restrict__ T, float* pts_out, float* nrm_out, int total) {
    // pts_out / nrm_out may be pts / nrm (in place): every element is read and written by the same thread, reads first
    const int s = blockIdx.y;
    const int lo = max(seg[s], 0), hi = min(seg[s + 1], total);
    const double* M = T + 16 * (long long)s;
    for (long long i = (long long)lo + blockIdx.x * 256 + threadIdx.x; i < hi; i += (long long)gridDim.x * 256) {
        const double p[3] = {(double)pts[4 * i], (double)pts[4 * i + 1], (double)pts[4 * i + 2]};
        const float inten = pts[4 * i + 3];
        double q[3] = {0.0, 0.0, 0.0};
        if (nrm) for (int c = 0; c < 3; ++c) q[c] = (double)nrm[3 * i + c];
        for (int r = 0; r < 3; ++r) {
            pts_out[4 * i + r] = (float)(((M[4 * r] * p[0] + M[4 * r + 1] * p[1]) + M[4 * r + 2] * p[2]) + M[4 * r + 3]);
            if (nrm) nrm_out[3 * i + r] = (float)((M[4 * r] * q[0] + M[4 * r + 1] * q[1]) + M[4 * r + 2] * q[2]);
        }
        pts_out[4 * i + 3] = inten;
    }
}

// ---------------------------------------------------------------- e. pose composition: one thread per frame
__global__ __launch_bounds__(64) void compose_poses_kernel(const double* A, const double* Bm, double* out, int n) {          // no __restrict__: out may be A or Bm
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n) return;
    const double* a = A + 16 * (long long)b;
    const double* m = Bm + 16 * (long long)b;
    double r[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double acc = __dmul_rn(a[4 * i], m[j]);
            for (int k = 1; k < 4; ++k) acc = __dadd_rn(acc, __dmul_rn(a[4 * i + k], m[4 * k + j]));
            r[4 * i + j] = acc;
        }
    for (int i = 0; i < 16; ++i) out[16 * (long long)b + i] = r[i];          // out may be A or Bm
}

const char* check_opt(const di2p_sample_opt_t* o, bool any_scale = false) {
    if (!o) return "null option block";
    if (o->mode < 0 || o->mode > 2) return "bad mode (0 train, 1 val, 2 val_random_Ry)";
    if (any_scale ? !(o->img_scale > 0.0 && o->img_scale <= 1.0) : (o->img_scale != 0.5 && o->img_scale != 1.0)) return "unsupported img_scale (0.5 or 1.0)";
    if (o->crop_top < 0 || o->img_H < 1 || o->img_W < 1 || o->Hs < 1 || o->Ws < 1) return "bad sizes";
    if (o->img_H > o->Hs || o->img_W > o->Ws) return "crop window larger than the scaled image";
    if ((long long)o->img_H * o->img_W > (1ll << 24)) return "crop window above 2^24 pixels";
    return nullptr;
}

}  // namespace

extern "C" int di2p_sample_draws(unsigned long long seed, const unsigned long long* seed_dev, int B, int frame0, const di2p_sample_opt_t* opt,
                                 const double* K, const double* Pc, const double* Pji, int32_t* ints, float* factors, double* Pr, double* PrPcn,
                                 float* P, float* K_out, void* stream) {
    const char* bad = check_opt(opt);
    DI2P_CHECK_ARG(!bad, bad);
    DI2P_CHECK_ARG(B >= 0 && frame0 >= 0, "bad sizes");
    DI2P_CHECK_ARG(B == 0 || (K && Pc && ints && factors && Pr && PrPcn && P && K_out), "null pointer");
    DI2P_CHECK_ARG(((uintptr_t)seed_dev & 7) == 0, "seed_dev must be 8-byte aligned");
    if (B == 0) return 0;
    hipLaunchKernelGGL(sample_draws_kernel, dim3(di2p_cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, seed, seed_dev, B, frame0, *opt, K, Pc, Pji, ints,
                       factors, Pr, PrPcn, P, K_out, (int)DS_KITTI, (int*)nullptr, (float*)nullptr);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_sample_draws_ds(unsigned long long seed, const unsigned long long* seed_dev, int B, int frame0, const di2p_sample_opt_t* opt,
                                    int dataset, const double* K, const double* P_cam_pc, int32_t* ints, float* factors, int32_t* color_enable,
                                    double* Pr, float* P, float* K_out, float* t_ij, void* stream) {
    const char* bad = check_opt(opt, true);
    DI2P_CHECK_ARG(!bad, bad);
    DI2P_CHECK_ARG(dataset == DS_OXFORD || dataset == DS_NUSCENES, "bad data set (1 Oxford, 2 nuScenes; KITTI frames go through di2p_sample_draws)");
    DI2P_CHECK_ARG(B >= 0 && frame0 >= 0, "bad sizes");
    DI2P_CHECK_ARG(B == 0 || (K && P_cam_pc && ints && factors && color_enable && Pr && P && K_out), "null pointer");
    DI2P_CHECK_ARG(((uintptr_t)seed_dev & 7) == 0, "seed_dev must be 8-byte aligned");
    if (B == 0) return 0;
    hipLaunchKernelGGL(sample_draws_kernel, dim3(di2p_cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, seed, seed_dev, B, frame0, *opt, K, P_cam_pc,
                       (const double*)nullptr, ints, factors, Pr, (double*)nullptr, P, K_out, dataset, color_enable, t_ij);
    DI2P_RETURN_LAUNCH();
}

extern "C" long long di2p_image_prepare_workspace_bytes(int B) { return B < 0 ? 0 : ((long long)B * 4 + 255) / 256 * 256 + 256; }

namespace {

// resize_k: 0 the scale of the option block (0.5: rounded 2x2 mean, 1.0: none), odd k >= 3: the centre pixel of every k x k block
int image_prepare(const uint8_t* images, int B, int H0, int W0, const di2p_sample_opt_t* opt, int crop_bottom, int resize_k, const int32_t* ints,
                  const float* factors, const int32_t* enable, int noflip, int geometry, int color, int reduce_blocks, float* out, void* workspace,
                  void* stream) {
    const char* bad = check_opt(opt, resize_k != 0);
    DI2P_CHECK_ARG(!bad, bad);
    DI2P_CHECK_ARG(crop_bottom >= 0 && (resize_k == 0 || (resize_k >= 3 && resize_k % 2 == 1)), "bad crop_bottom / resize_k (0, or odd >= 3)");
    DI2P_CHECK_ARG(geometry || (crop_bottom == 0 && resize_k == 0), "crop_bottom and resize_k need geometry");
    DI2P_CHECK_ARG(B >= 0 && H0 >= 1 && W0 >= 1 && reduce_blocks >= 0 && reduce_blocks <= 65535 && B <= 65535, "bad sizes");
    DI2P_CHECK_ARG((long long)H0 * W0 * 3 < (1ll << 31), "image above 2^31 bytes");
    ImgGeom g{H0, W0, 0, 0, opt->img_H, opt->img_W, 0, 0, 1, noflip};
    if (geometry) {
        const bool half = resize_k == 0 && opt->img_scale == 0.5;
        const int div = resize_k ? resize_k : half ? 2 : 1;
        DI2P_CHECK_ARG(opt->crop_top < H0 - crop_bottom, "crop_original_top_rows / crop_original_bottom_rows leave no image");
        const int Hc = H0 - opt->crop_top - crop_bottom;
        DI2P_CHECK_ARG(!half || (Hc % 2 == 0 && W0 % 2 == 0), "odd scaled size: img_scale 0.5 needs even cropped source dimensions");
        DI2P_CHECK_ARG(Hc % div == 0 && W0 % div == 0, "resize_k must divide both cropped source dimensions");
        DI2P_CHECK_ARG(opt->Hs == Hc / div && opt->Ws == W0 / div, "scaled size does not match the source image");
        g.top = opt->crop_top; g.half = half ? 1 : 0; g.k = resize_k ? resize_k : 1; g.max_dx = opt->Ws - opt->img_W; g.max_dy = opt->Hs - opt->img_H;
    } else {
        DI2P_CHECK_ARG(H0 == opt->img_H && W0 == opt->img_W, "without geometry the source must already be img_H x img_W");
    }
    DI2P_CHECK_ARG(B == 0 || (images && out && workspace), "null pointer (images, out, workspace)");
    DI2P_CHECK_ARG(B == 0 || !(geometry || color) || (ints && factors), "null draw table");
    DI2P_CHECK_ARG(((uintptr_t)workspace & 3) == 0, "workspace must be 4-byte aligned");
    if (B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int npix = g.H * g.W;
    unsigned* sums = (unsigned*)workspace;
    if (color) {
        // zeroed by a launch, not by hipMemsetAsync: replayed from a captured graph the memset node was seen NOT to order before the
        // reduction (second replay of a 20-frame plan: stale sums, a wrong contrast mean); kernel nodes keep their order
        hipLaunchKernelGGL(zero_sums_kernel, dim3(di2p_cdiv(B, 256)), dim3(256), 0, st, sums, B);
        const int rb = reduce_blocks > 0 ? reduce_blocks : min(di2p_cdiv(npix, 1024), 128);
        hipLaunchKernelGGL(grey_sum_kernel, dim3(rb, B), dim3(256), 0, st, images, g, ints, factors, enable, geometry, sums);
    }
    hipLaunchKernelGGL(image_apply_kernel, dim3(di2p_cdiv(npix, 256), B), dim3(256), 0, st, images, g, ints, factors, enable, geometry, color, sums,
                       out);
    DI2P_RETURN_LAUNCH();
}

}  // namespace

extern "C" int di2p_image_prepare(const uint8_t* images, int B, int H0, int W0, const di2p_sample_opt_t* opt, const int32_t* ints,
                                  const float* factors, int geometry, int color, int reduce_blocks, float* out, void* workspace, void* stream) {
    return image_prepare(images, B, H0, W0, opt, 0, 0, ints, factors, nullptr, 0, geometry, color, reduce_blocks, out, workspace, stream);
}

extern "C" int di2p_image_prepare_ds(const uint8_t* images, int B, int H0, int W0, const di2p_sample_opt_t* opt, int crop_bottom, int resize_k,
                                     const int32_t* ints, const float* factors, const int32_t* color_enable, int color, int reduce_blocks,
                                     float* out, void* workspace, void* stream) {
    return image_prepare(images, B, H0, W0, opt, crop_bottom, resize_k, ints, factors, color_enable, 1, 1, color, reduce_blocks, out, workspace, stream);
}

extern "C" int di2p_transform_segments(const float* points, const float* normals, const int32_t* seg_offsets, const double* transforms, int S,
                                       int total, float* points_out, float* normals_out, void* stream) {
    DI2P_CHECK_ARG(S >= 0 && S <= 65535 && total >= 0, "bad sizes (S <= 65535)");
    DI2P_CHECK_ARG(S == 0 || total == 0 || (points && seg_offsets && transforms && points_out), "null pointer");
    DI2P_CHECK_ARG(!normals == !normals_out, "normals and normals_out go together");
    if (S == 0 || total == 0) return 0;
    const int blocks = max(1, min(di2p_cdiv(di2p_cdiv(total, S), 256), 256));
    hipLaunchKernelGGL(transform_segments_kernel, dim3(blocks, S), dim3(256), 0, (hipStream_t)stream, points, normals, seg_offsets, transforms,
                       points_out, normals_out, total);
    DI2P_RETURN_LAUNCH();
}

extern "C" int di2p_compose_poses(const double* A, const double* Bm, int n, double* out, void* stream) {
    DI2P_CHECK_ARG(n >= 0, "bad size");
    DI2P_CHECK_ARG(n == 0 || (A && Bm && out), "null pointer");
    if (n == 0) return 0;
    hipLaunchKernelGGL(compose_poses_kernel, dim3(di2p_cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, A, Bm, out, n);
    DI2P_RETURN_LAUNCH();
}
