// waymo_sweep.hip -- a Waymo top-lidar range image (polar, sensor frame, per-pixel pose) -> the sweep the detector eats
// (Cartesian, vehicle frame at the frame's timestamp).  Restates what the reference's offline exporter
// (converters/waymo/export.py:55-147 `convert_range_image_to_cartesian`) asks of waymo_open_dataset's
// range_image_utils.extract_point_cloud_from_range_image / compute_inclination / transform_utils.get_rotation_matrix; the
// semantics are DECLARED in include/rv3d.h (neither TensorFlow nor waymo_open_dataset exists where this is built: they are not
// pinned against those binaries).
//
//   one thread per OUTPUT pixel (b, row, padded column); grid = (ceil(Wp / 256), H, B): row and frame are uniform per workgroup,
//   so the extrinsic, the inverse frame pose and the row's inclination are uniform loads.  The 16-byte range-image pixel is one
//   vector load, the 24-byte pixel pose three 8-byte loads.  All arithmetic fp64, rounded to fp32 once.  Invalid pixels
//   (range <= 0, NaN range, nlz == 1) take no arithmetic at all and leave +0.0: a select, not a product with a 0/1 mask.
//   Two outputs over the one device function:
//     sweep  (B, H, W, 6) channel-last [range, intensity, elongation, x, y, z] -- the reference's table (three 8-byte stores);
//     batch  features (B, F, H, Wp), cart (B, 3, H, Wp), mask (B, 1, H, Wp) u8 with the W padding of subsample_range_view done in
//            the same pass (planar stores, coalesced along W; a wrapped column of `circular` recomputes its source pixel).
//   40 B read + 24 B (sweep) or 37 B (Waymo batch: 6 features, 3 coordinates, 1 mask byte) written per pixel; HBM- and launch-bound.
#include "common.h"

namespace {

struct WaymoArgs {
    const float* range_image;      // (B, H, W, 4)
    const double* extrinsic;       // (B, 4, 4)
    const double* inclination;     // (B, H), by image row
    const float* pixel_pose;       // (B, H, W, 6) or null
    const double* inv_frame_pose;  // (B, 3, 4) or null
    int32_t H, W;
    int32_t pad, circular;  // batch only
    int32_t n_feat;
    int32_t feat_src[16], feat_op[16];
    float* sweep;     // sweep mode
    float* features;  // batch mode
    float* cart;
    uint8_t* mask;
    unsigned long long* num_pts;  // (B) or null; zeroed by the entry point
};

struct Pixel {
    float ch[6];  // range, intensity, elongation, x, y, z
    bool valid;
};

// the declared per-pixel semantics (include/rv3d.h): source pixel (b, r, c) -> the six sweep channels
__device__ __forceinline__ Pixel waymo_pixel(const WaymoArgs& a, int b, int r, int c) {
    Pixel p;
    const int64_t pix = ((int64_t)b * a.H + r) * a.W + c;
    const f32x4 ri = *reinterpret_cast<const f32x4*>(a.range_image + 4 * pix);
    p.valid = ri[0] > 0.f && ri[3] != 1.0f;
#pragma unroll
    for (int k = 0; k < 6; ++k) p.ch[k] = 0.f;
    if (!p.valid) return p;
    const double* E = a.extrinsic + 16 * (int64_t)b;
    const double az_correction = atan2(E[4], E[0]);
    const double ratio = ((double)a.W - (double)c - 0.5) / (double)a.W;
    const double az = (2.0 * ratio - 1.0) * 3.141592653589793238 - az_correction;
    const double incl = a.inclination[(int64_t)b * a.H + r];
    double sa, ca, si, ci;
    sincos(az, &sa, &ca);
    sincos(incl, &si, &ci);
    const double rng = (double)ri[0];
    const double s[3] = {rng * (ca * ci), rng * (sa * ci), rng * si};
    double v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = E[4 * k] * s[0] + E[4 * k + 1] * s[1] + E[4 * k + 2] * s[2] + E[4 * k + 3];
    if (a.pixel_pose) {
        const float2* pp = reinterpret_cast<const float2*>(a.pixel_pose + 6 * pix);
        const float2 rp = pp[0], yt = pp[1], tt = pp[2];  // (roll, pitch) (yaw, tx) (ty, tz)
        double sr, cr, sp, cp, sy, cy;
        sincos((double)rp.x, &sr, &cr);
        sincos((double)rp.y, &sp, &cp);
        sincos((double)yt.x, &sy, &cy);
        // R = Rz(yaw) Ry(pitch) Rx(roll)
        const double R[9] = {cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr,
                             sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr,
                             -sp,     cp * sr,                cp * cr};
        const double t[3] = {(double)yt.y, (double)tt.x, (double)tt.y};
        double w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = R[3 * k] * v[0] + R[3 * k + 1] * v[1] + R[3 * k + 2] * v[2] + t[k];
        const double* V = a.inv_frame_pose + 12 * (int64_t)b;
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = V[4 * k] * w[0] + V[4 * k + 1] * w[1] + V[4 * k + 2] * w[2] + V[4 * k + 3];
    }
    p.ch[0] = ri[0];
    p.ch[1] = ri[1];
    p.ch[2] = ri[2];
    p.ch[3] = (float)v[0];
    p.ch[4] = (float)v[1];
    p.ch[5] = (float)v[2];
    return p;
}

// one atomic per wave; an integer sum, so the order does not matter
__device__ __forceinline__ void count_valid(const WaymoArgs& a, int b, bool counted) {
    if (!a.num_pts) return;
    const unsigned long long votes = __ballot(counted);
    if (votes && (threadIdx.x & 63) == 0) atomicAdd(a.num_pts + b, (unsigned long long)__popcll(votes));
}

__global__ __launch_bounds__(256) void waymo_sweep_kernel(const WaymoArgs a) {
    const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y, b = blockIdx.z;
    const bool inside = c < a.W;
    Pixel p;
    p.valid = false;
    if (inside) {
        p = waymo_pixel(a, b, r, c);
        float2* dst = reinterpret_cast<float2*>(a.sweep + 6 * (((int64_t)b * a.H + r) * a.W + c));
        dst[0] = make_float2(p.ch[0], p.ch[1]);
        dst[1] = make_float2(p.ch[2], p.ch[3]);
        dst[2] = make_float2(p.ch[4], p.ch[5]);
    }
    count_valid(a, b, inside && p.valid);
}

__global__ __launch_bounds__(256) void waymo_batch_kernel(const WaymoArgs a) {
    const int Wp = a.W + 2 * a.pad;
    const int wp = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y, b = blockIdx.z;
    const bool inside = wp < Wp;
    int c = wp - a.pad;
    const bool own = inside && c >= 0 && c < a.W;  // a column of the image itself (not a wrapped or zero one): counted in num_pts
    if (a.circular) c = (c % a.W + a.W) % a.W;
    Pixel p;
    p.valid = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) p.ch[k] = 0.f;
    if (inside && c >= 0 && c < a.W) p = waymo_pixel(a, b, r, c);
    if (inside) {
        const int64_t plane = (int64_t)a.H * Wp, at = (int64_t)r * Wp + wp;
        float* f = a.features + (int64_t)b * a.n_feat * plane + at;
        for (int k = 0; k < a.n_feat; ++k) {
            const int src = a.feat_src[k];
            float v = src == 0 ? p.ch[0] : src == 1 ? p.ch[1] : src == 2 ? p.ch[2] : src == 3 ? p.ch[3] : src == 4 ? p.ch[4] : p.ch[5];
            if (a.feat_op[k] == 1) v = rv_feature_tanh(v);
            f[k * plane] = p.valid ? v : 0.f;
        }
        float* xyz = a.cart + (int64_t)b * 3 * plane + at;
        xyz[0] = p.ch[3];
        xyz[plane] = p.ch[4];
        xyz[2 * plane] = p.ch[5];
        a.mask[(int64_t)b * plane + at] = p.valid ? 1 : 0;
    }
    count_valid(a, b, own && p.valid);
}

int fill_common(WaymoArgs& a, const char* who, const float* range_image, const double* extrinsic, const double* inclination,
                const float* pixel_pose, const double* inv_frame_pose, int32_t B, int32_t H, int32_t W, int64_t* num_pts) {
    RV_REQUIRE(range_image && extrinsic && inclination, "%s: null argument (range_image, extrinsic and inclination are required)", who);
    RV_REQUIRE(B > 0 && H > 0 && W > 0, "%s: empty image (B %d, H %d, W %d)", who, B, H, W);
    RV_REQUIRE(B <= 65535 && H <= 65535, "%s: B %d / H %d beyond the launch grid (65535 each)", who, B, H);
    RV_REQUIRE((pixel_pose != nullptr) == (inv_frame_pose != nullptr),
               "%s: pixel_pose and inv_frame_pose go together (a per-pixel pose needs the inverse frame pose, and the reverse)", who);
    RV_REQUIRE(((uintptr_t)range_image & 15) == 0 && ((uintptr_t)pixel_pose & 7) == 0 && ((uintptr_t)extrinsic & 7) == 0 &&
                   ((uintptr_t)inclination & 7) == 0 && ((uintptr_t)inv_frame_pose & 7) == 0 && ((uintptr_t)num_pts & 7) == 0,
               "%s: range_image must be 16-byte aligned, the other inputs 8-byte aligned", who);
    a.range_image = range_image;
    a.extrinsic = extrinsic;
    a.inclination = inclination;
    a.pixel_pose = pixel_pose;
    a.inv_frame_pose = inv_frame_pose;
    a.H = H;
    a.W = W;
    a.pad = a.circular = a.n_feat = 0;
    a.sweep = a.features = a.cart = nullptr;
    a.mask = nullptr;
    a.num_pts = reinterpret_cast<unsigned long long*>(num_pts);
    return 0;
}

}  // namespace

extern "C" int rv_waymo_range_image_to_sweep(const float* range_image, const double* extrinsic, const double* inclination,
                                             const float* pixel_pose, const double* inv_frame_pose, int32_t B, int32_t H, int32_t W,
                                             float* sweep, int64_t* num_pts, rvStream stream) {
    WaymoArgs a;
    if (fill_common(a, "rv_waymo_range_image_to_sweep", range_image, extrinsic, inclination, pixel_pose, inv_frame_pose, B, H, W, num_pts)) return 1;
    RV_REQUIRE(sweep && ((uintptr_t)sweep & 7) == 0, "rv_waymo_range_image_to_sweep: null or misaligned sweep (8-byte aligned)");
    a.sweep = sweep;
    if (num_pts && hipMemsetAsync(num_pts, 0, sizeof(int64_t) * B, (hipStream_t)stream) != hipSuccess)
        RV_FAIL("rv_waymo_range_image_to_sweep: clearing num_pts: %s", hipGetErrorString(hipGetLastError()));
    hipLaunchKernelGGL(waymo_sweep_kernel, dim3((unsigned)rv_ceil_div(W, 256), (unsigned)H, (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
    RV_CHECK_LAUNCH("waymo_sweep_kernel");
    return 0;
}

extern "C" int rv_waymo_range_image_to_batch(const float* range_image, const double* extrinsic, const double* inclination,
                                             const float* pixel_pose, const double* inv_frame_pose, int32_t B, int32_t H, int32_t W,
                                             int32_t n_feat, const int32_t* host_feat_src, const int32_t* host_feat_op, int32_t pad,
                                             int32_t circular, float* features, float* cart, uint8_t* mask, int64_t* num_pts,
                                             rvStream stream) {
    WaymoArgs a;
    if (fill_common(a, "rv_waymo_range_image_to_batch", range_image, extrinsic, inclination, pixel_pose, inv_frame_pose, B, H, W, num_pts)) return 1;
    RV_REQUIRE(host_feat_src && host_feat_op && features && cart && mask, "rv_waymo_range_image_to_batch: null argument");
    RV_REQUIRE(n_feat >= 1 && n_feat <= 16, "rv_waymo_range_image_to_batch: %d features (1..16)", n_feat);
    RV_REQUIRE(pad >= 0 && (int64_t)W + 2 * (int64_t)pad <= 0x7fffff00, "rv_waymo_range_image_to_batch: bad pad %d", pad);
    for (int f = 0; f < n_feat; ++f) {
        RV_REQUIRE(host_feat_src[f] >= 0 && host_feat_src[f] <= 5, "rv_waymo_range_image_to_batch: feature %d: source %d is not a sweep channel (0..5)",
                   f, host_feat_src[f]);
        RV_REQUIRE(host_feat_op[f] == 0 || host_feat_op[f] == 1, "rv_waymo_range_image_to_batch: feature %d: op %d (0 copy, 1 tanh)", f, host_feat_op[f]);
        a.feat_src[f] = host_feat_src[f];
        a.feat_op[f] = host_feat_op[f];
    }
    a.n_feat = n_feat;
    a.pad = pad;
    a.circular = circular ? 1 : 0;
    a.features = features;
    a.cart = cart;
    a.mask = mask;
    if (num_pts && hipMemsetAsync(num_pts, 0, sizeof(int64_t) * B, (hipStream_t)stream) != hipSuccess)
        RV_FAIL("rv_waymo_range_image_to_batch: clearing num_pts: %s", hipGetErrorString(hipGetLastError()));
    hipLaunchKernelGGL(waymo_batch_kernel, dim3((unsigned)rv_ceil_div((int64_t)W + 2 * pad, 256), (unsigned)H, (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, a);
    RV_CHECK_LAUNCH("waymo_batch_kernel");
    return 0;
}
