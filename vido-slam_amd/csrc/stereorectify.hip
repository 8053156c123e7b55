// stereorectify.hip — remap of one or two raw camera images through rectification maps, on gfx950 (no reference counterpart: the reference's datasets are rectified or
// it undistorts points only, Frame.cc:603-633).  Rule (include/vido_c.h; the numpy statement is tests/refimpl/stereo_rectify_np.py): a map entry (mx, my) in
// 1/256 px is inside iff 0 <= mx <= (sw - 1) 256 and 0 <= my <= (sh - 1) 256; an inside pixel is the bilinear mean of its four neighbours with the weights' products kept
// whole, (sum + 32768) >> 16 (the sum stays below 2^31), x1 / y1 clamped to the last column / row; any other pixel is 0 in every channel, and reads no source byte.
// One launch for both cameras (blockIdx.z), no LDS, no atomics, no scratch.  A thread owns 4 consecutive pixels of a destination row: their 8 map words come as two
// 16-byte loads when their address is 16-byte aligned (always with a 16-byte aligned map and an even dst_w), the source bytes through plain read-only loads (the images
// stay in L2), and the 4 pixels leave in the widest stores their address allows: a dword (1 channel), three dwords (3) or 16 bytes (4); bytes otherwise and for the
// last dst_w % 4 pixels of a row.  Integers only: no execution order matters.
#include "common.hpp"

struct RectifyArgs {
    const uint8_t* src[2]; const int32_t* map[2]; uint8_t* dst[2]; uint8_t* inside[2];
    int sw, sh, dw, dh, groups;                                    // groups = ceil(dw / 4): threads per row
    long long sstride, dstride;
};

// the CN bytes of one destination pixel; 0 and *in = 0 outside
template <int CN>
__device__ __forceinline__ void rc_pixel(const uint8_t* __restrict__ src, long long sstride, int sw, int sh, int mx, int my, uint8_t* out, uint8_t* in)
{
    const bool inside = mx >= 0 && mx <= (sw - 1) * 256 && my >= 0 && my <= (sh - 1) * 256;
    *in = inside ? 1 : 0;
#pragma unroll
    for (int c = 0; c < CN; c++) out[c] = 0;
    if (!inside) return;
    const int x0 = mx >> 8, y0 = my >> 8;
    const unsigned ax = mx & 255, ay = my & 255;
    const int x1 = min(x0 + 1, sw - 1), y1 = min(y0 + 1, sh - 1);
    const uint8_t* r0 = src + (long long)y0 * sstride;
    const uint8_t* r1 = src + (long long)y1 * sstride;
    const unsigned w00 = (256 - ax) * (256 - ay), w01 = ax * (256 - ay), w10 = (256 - ax) * ay, w11 = ax * ay;
#pragma unroll
    for (int c = 0; c < CN; c++) {
        const unsigned a = r0[x0 * CN + c], b = r0[x1 * CN + c], d = r1[x0 * CN + c], e = r1[x1 * CN + c];
        out[c] = (uint8_t)((w00 * a + w01 * b + w10 * d + w11 * e + 32768u) >> 16);
    }
}

template <int CN>
__global__ __launch_bounds__(256) void k_rectify(RectifyArgs A)
{
    const int cam = blockIdx.z;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= (unsigned)A.groups * (unsigned)A.dh) return;
    const int row = t / (unsigned)A.groups, x = 4 * (int)(t % (unsigned)A.groups);
    const uint8_t* __restrict__ src = A.src[cam];
    const int32_t* __restrict__ mp = A.map[cam] + 2 * ((size_t)row * A.dw + x);
    uint8_t* dst = A.dst[cam] + (long long)row * A.dstride + (long long)x * CN;
    uint8_t* ins = A.inside[cam] ? A.inside[cam] + (size_t)row * A.dw + x : nullptr;
    if (x + 4 <= A.dw) {
        int m[8];
        if (((uintptr_t)mp & 15) == 0) {
            const int4 a = *reinterpret_cast<const int4*>(mp), b = *reinterpret_cast<const int4*>(mp + 4);
            m[0] = a.x; m[1] = a.y; m[2] = a.z; m[3] = a.w; m[4] = b.x; m[5] = b.y; m[6] = b.z; m[7] = b.w;
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) m[k] = mp[k];
        }
        union { uint8_t b[4 * CN]; uint32_t w[CN]; } px;
        union { uint8_t b[4]; uint32_t w; } in;
#pragma unroll
        for (int k = 0; k < 4; k++) rc_pixel<CN>(src, A.sstride, A.sw, A.sh, m[2 * k], m[2 * k + 1], px.b + k * CN, in.b + k);
        bool wide = false;
        if constexpr (CN == 4) {
            wide = ((uintptr_t)dst & 15) == 0;
            if (wide) *reinterpret_cast<uint4*>(dst) = make_uint4(px.w[0], px.w[1], px.w[2], px.w[3]);
        }
        if (wide) {
        } else if (((uintptr_t)dst & 3) == 0) {
#pragma unroll
            for (int k = 0; k < CN; k++) reinterpret_cast<uint32_t*>(dst)[k] = px.w[k];
        } else {
#pragma unroll
            for (int k = 0; k < 4 * CN; k++) dst[k] = px.b[k];
        }
        if (ins) {
            if (((uintptr_t)ins & 3) == 0) *reinterpret_cast<uint32_t*>(ins) = in.w;
            else { ins[0] = in.b[0]; ins[1] = in.b[1]; ins[2] = in.b[2]; ins[3] = in.b[3]; }
        }
    } else {
        for (int k = 0; x + k < A.dw; k++) {                        // the last dst_w % 4 pixels of the row
            uint8_t b[CN], in;
            rc_pixel<CN>(src, A.sstride, A.sw, A.sh, mp[2 * k], mp[2 * k + 1], b, &in);
#pragma unroll
            for (int c = 0; c < CN; c++) dst[k * CN + c] = b[c];
            if (ins) ins[k] = in;
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------
static bool rc_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    return a && b && (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}

extern "C" int vido_rectify(vido_ctx* ctx, const uint8_t* src0, const uint8_t* src1, int channels, int src_stride, int src_w, int src_h, const int32_t* map0, const int32_t* map1,
                            int dst_w, int dst_h, uint8_t* dst0, uint8_t* dst1, int dst_stride, uint8_t* inside0_out, uint8_t* inside1_out, int on_device)
{
    if (!ctx) return VIDO_E_INVALID;
    if (!src0 || !map0 || !dst0) return vido_set_error(ctx, VIDO_E_INVALID, "rectify: null image, map or destination of the first camera");
    const bool two = src1 != nullptr;
    if ((map1 != nullptr) != two || (dst1 != nullptr) != two) return vido_set_error(ctx, VIDO_E_INVALID, "rectify: src1, map1 and dst1 are given together or not at all");
    if (inside1_out && !two) return vido_set_error(ctx, VIDO_E_INVALID, "rectify: inside1_out without a second camera");
    if (channels != 1 && channels != 3 && channels != 4) return vido_set_error(ctx, VIDO_E_INVALID, "rectify: %d channels, 1, 3 or 4 expected", channels);
    if (src_w < 16 || src_h < 16 || src_w > 4095 || src_h > 4095 || dst_w < 16 || dst_h < 16 || dst_w > 4095 || dst_h > 4095)
        return vido_set_error(ctx, VIDO_E_INVALID, "rectify: size %d x %d -> %d x %d outside 16 .. 4095", src_w, src_h, dst_w, dst_h);
    if (src_stride < src_w * channels || dst_stride < dst_w * channels)
        return vido_set_error(ctx, VIDO_E_INVALID, "rectify: stride %d / %d below the row's %d / %d bytes", src_stride, dst_stride, src_w * channels, dst_w * channels);
    const size_t px = (size_t)dst_w * dst_h;
    const size_t sbytes = (size_t)(src_h - 1) * src_stride + (size_t)src_w * channels, dbytes = (size_t)(dst_h - 1) * dst_stride + (size_t)dst_w * channels, mbytes = px * 8;
    {
        const void* ins[4] = {src0, src1, map0, map1}; const size_t nin[4] = {sbytes, sbytes, mbytes, mbytes};
        void* outs[4] = {dst0, dst1, inside0_out, inside1_out}; const size_t nout[4] = {dbytes, dbytes, px, px};
        for (int o = 0; o < 4; o++) {
            for (int i = 0; i < 4; i++) if (rc_overlap(outs[o], nout[o], ins[i], nin[i])) return vido_set_error(ctx, VIDO_E_INVALID, "rectify: a destination overlaps a source");
            for (int q = o + 1; q < 4; q++) if (outs[o] && outs[o] == outs[q]) return vido_set_error(ctx, VIDO_E_INVALID, "rectify: two destinations are one");
        }
    }
    if (on_device && ((((uintptr_t)map0 | (uintptr_t)map1) & 3) != 0)) return vido_set_error(ctx, VIDO_E_INVALID, "rectify: the device maps must be 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = on_device && ctx->has_ext_stream ? ctx->ext_stream : ctx->stream;
    if (!on_device) {                                                      // the host form: from here on the pointers are their slots of the staging buffer
        HostStaging& T = ctx->staging;                                     // (the destinations go up too: the bytes between their rows come back as they were)
        const uint8_t *d0 = dst0, *d1 = dst1;
        T.begin(); T.in(&src0, sbytes); T.in(&src1, sbytes); T.in(&map0, mbytes); T.in(&map1, mbytes); T.out(&inside0_out, px); T.out(&inside1_out, px);
        T.inout(&d0, &dst0, dbytes); T.inout(&d1, &dst1, dbytes);
        if (int rc = staging_upload(ctx, st)) return rc;
    }
    RectifyArgs A;
    A.src[0] = src0; A.src[1] = src1; A.map[0] = map0; A.map[1] = map1; A.dst[0] = dst0; A.dst[1] = dst1; A.inside[0] = inside0_out; A.inside[1] = inside1_out;
    A.sw = src_w; A.sh = src_h; A.dw = dst_w; A.dh = dst_h; A.groups = (dst_w + 3) / 4; A.sstride = src_stride; A.dstride = dst_stride;
    const dim3 grid(((unsigned)A.groups * (unsigned)dst_h + 255u) / 256u, 1, two ? 2 : 1);
    if (channels == 1) hipLaunchKernelGGL(k_rectify<1>, grid, dim3(256), 0, st, A);
    else if (channels == 3) hipLaunchKernelGGL(k_rectify<3>, grid, dim3(256), 0, st, A);
    else hipLaunchKernelGGL(k_rectify<4>, grid, dim3(256), 0, st, A);
    HIP_TRY(ctx, hipGetLastError());
    if (!on_device) return staging_download(ctx, st);
    return VIDO_OK;
}
