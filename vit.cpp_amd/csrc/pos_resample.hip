// pos_resample.hip -- the position-embedding table of a context whose img_size differs from the file's (vitx_op_pos_embed_resample).
//
// A plain streaming kernel: it runs once per context, not per forward.  One thread per output row x V channels (V = 4 with 16-byte loads
// and stores when D % 4 == 0 and the pointers allow it, else 1); consecutive threads take consecutive channel groups of one row, so a
// wave's loads of one tap are contiguous.  Row 0 (the class token) is copied.  Tap indices and weights come from pos_resample.h, the
// definition the host loop shares: same operations in the same order, no FMA contraction -- the same bits.
#include "kernels.h"
#include "model_file.h"
#include "pos_resample.h"

namespace vitx {

namespace {

template <int V>
__global__ __launch_bounds__(256) void pos_resample_kernel(const float *__restrict__ pos, float *__restrict__ out, int gy_in, int gx_in, int D, int gy_out,
                                                           int gx_out, int interp, float scale_y, float scale_x, unsigned total) {
    const unsigned tid = blockIdx.x * 256u + threadIdx.x;
    if (tid >= total) return;
    const unsigned groups = (unsigned)D / V, row = tid / groups;
    const int d = (int)(tid - row * groups) * V;
    float v[V];
    if (row == 0) {
#pragma unroll
        for (int e = 0; e < V; ++e) v[e] = pos[d + e];
    } else {
        const int cell = (int)row - 1, oy = cell / gx_out, ox = cell - oy * gx_out;
        const PosAxis ay = pos_axis(interp, gy_in, gy_out, scale_y, oy), ax = pos_axis(interp, gx_in, gx_out, scale_x, ox);
        pos_cell<V>(pos + D, gy_in, gx_in, D, interp, ay, ax, d, v);
    }
    float *o = out + (size_t)row * D + d;
    if constexpr (V == 4) { pos_f32x4 q; q[0] = v[0]; q[1] = v[1]; q[2] = v[2]; q[3] = v[3]; *(pos_f32x4 *)o = q; }
    else o[0] = v[0];
}

}  // namespace

hipError_t launch_pos_resample(const float *pos, int gy_in, int gx_in, int D, int gy_out, int gx_out, int interp, float *out, hipStream_t stream) {
    const size_t rows_out = (size_t)gy_out * gx_out + 1;
    if (gy_in == gy_out && gx_in == gx_out) return hipMemcpyAsync(out, pos, rows_out * D * 4, hipMemcpyDeviceToDevice, stream);
    const float sy = pos_scale(gy_in, gy_out), sx = pos_scale(gx_in, gx_out);
    const bool vec = D % 4 == 0 && (((uintptr_t)pos | (uintptr_t)out) & 15) == 0;
    const unsigned total = (unsigned)(rows_out * (size_t)(vec ? D / 4 : D));
    const unsigned blocks = (total + 255u) / 256u;
    if (vec) hipLaunchKernelGGL(pos_resample_kernel<4>, dim3(blocks), dim3(256), 0, stream, pos, out, gy_in, gx_in, D, gy_out, gx_out, interp, sy, sx, total);
    else hipLaunchKernelGGL(pos_resample_kernel<1>, dim3(blocks), dim3(256), 0, stream, pos, out, gy_in, gx_in, D, gy_out, gx_out, interp, sy, sx, total);
    return hipGetLastError();
}

}  // namespace vitx

extern "C" int vitx_op_pos_embed_resample(const void *d_pos, int gy_in, int gx_in, int D, int gy_out, int gx_out, int interp, void *d_out, void *stream) {
    if (!vitx::pos_resample_args_ok(d_pos, gy_in, gx_in, D, gy_out, gx_out, interp, d_out)) { vitx::set_error("vitx_op_pos_embed_resample: invalid argument"); return VITX_ERR_ARG; }
    const hipError_t e = vitx::launch_pos_resample((const float *)d_pos, gy_in, gx_in, D, gy_out, gx_out, interp, (float *)d_out, (hipStream_t)stream);
    if (e != hipSuccess) { vitx::set_error("vitx_op_pos_embed_resample: %s", hipGetErrorString(e)); return VITX_ERR_HIP; }
    return VITX_OK;
}
