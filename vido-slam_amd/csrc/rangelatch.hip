// rangelatch.hip — the split-fp16 range flag: its host-side read (vido_conv1x1_range_flag) and its per-frame latch (vido_range_latch).
//
// The split-fp16 kernels (conv1x1.hip 1x1 and 2x2 transposed, conv3x3h.hip, fch.hip) OR 1 into the context's pinned flag word when a launch met |x| >= 65504, an infinity or
// a NaN.  Read on the host, that word says "some launch since the last reset" — with the networks of frame k + 1 already queued behind frame k, that cannot name the frame.
// The latch is a one-lane launch in STREAM ORDER: it moves the flag into a word of the caller's (flag -> 0, *dst |= old), so that *dst holds exactly the trips of the launches
// enqueued before it on that stream (and of any other stream the caller has joined), and the flag starts again at 0 for the launches after it.
#include "common.hpp"

/* The range flag of the split-fp16 kernels (1x1, 3x3, grouped 3x3, fully connected, 2x2 transposed): non-zero when a launch since the last reset met an activation with
 * |x| >= 65504, an infinity or a NaN — its outputs are then not valid.
 * Host-visible memory written by the kernels: read it after the stream has been waited for.  reset != 0 clears it. */
int vido_conv1x1_range_flag(vido_ctx* ctx, int reset)
{
    if (!ctx || !ctx->c1_range_flag) return 0;
    // read and reset in ONE atomic step: a flag raised between a load and a store would be lost
    return reset ? (int)__atomic_exchange_n(ctx->c1_range_flag, 0u, __ATOMIC_ACQ_REL) : (int)__atomic_load_n(ctx->c1_range_flag, __ATOMIC_ACQUIRE);
}

__global__ void k_range_latch(unsigned* flag, unsigned* dst)
{
    if (threadIdx.x != 0) return;
    const unsigned old = atomicExch_system(flag, 0u);      // system scope: the flag is host memory, the split kernels raise it with atomicOr
    if (old) atomicOr_system(dst, old);                      // dst: a pinned host word or a device word; nothing is written when nothing tripped
}

int vido_range_latch(vido_ctx* ctx, unsigned* dst)
{
    if (!ctx) return VIDO_E_INVALID;
    if (!dst) return vido_set_error(ctx, VIDO_E_INVALID, "range_latch: dst is null");
    if (!ctx->c1_range_flag) return vido_set_error(ctx, VIDO_E_HIP, "range_latch: the context has no range flag (its pinned word could not be allocated)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->has_ext_stream ? ctx->ext_stream : ctx->stream;
    hipLaunchKernelGGL(k_range_latch, dim3(1), dim3(64), 0, st, ctx->c1_range_flag, dst);
    HIP_TRY(ctx, hipGetLastError());
    return VIDO_OK;
}
