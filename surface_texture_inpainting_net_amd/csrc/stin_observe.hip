// Observer masks on the device: which vertices does every camera pose of a scan see (reference
// preprocessing/observed_texture_map_generation.py :159-267, `generate_masks.sh observers`; the reference renders the mesh with
// PyTorch3D's MeshRasterizer and keeps pix_to_face).  Contract: include/stin_hip.h ("observer masks"); tests/_observers_oracle.py
// restates it in numpy, pixel-major, and agrees bit for bit.
//
//   faces, and per batch of poses clear, transform, raster, large: the shared rasteriser (stin_raster.hip) with the square screen
//              of the contract; the z-buffers of a batch live in the workspace.
//   resolve:   one thread per (pixel, pose): the winning face's three vertices get bit p of their row (atomicOr on uint32, after a
//              plain look that skips the bits already there).
// Integer min / or only: the result does not depend on the schedule, the batch size or `large_box`.
#include "stin_raster.h"

namespace {

constexpr int OB = 256;                                   // threads per workgroup
constexpr int LARGE_GRID = 1024;                          // workgroups of the large-face kernel (r20_observers.md)

RasterLayout observe_layout(int64_t N, int64_t F, int S, int batch) {
    return stin_raster_layout(N, F, batch, (size_t)batch * (size_t)S * (size_t)S);
}

__global__ void k_observe_resolve(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ f32, int64_t S2, int64_t p0,
                                  uint32_t* __restrict__ bits, int64_t words) {
    const int64_t i = (int64_t)blockIdx.x * OB + threadIdx.x;
    if (i >= S2) return;
    const unsigned long long key = keys[(int64_t)blockIdx.y * S2 + i];
    if (key == STIN_RASTER_NO_FACE) return;
    const int64_t f = (int64_t)(key & 0xffffffffull);
    const int64_t p = p0 + blockIdx.y;
    const uint32_t bit = 1u << (p & 31);
    for (int k = 0; k < 3; ++k) {
        uint32_t* w = bits + (int64_t)f32[3 * f + k] * words + (p >> 5);
        if (!(*w & bit)) atomicOr(w, bit);
    }
}

__global__ void k_observe_mask(const uint32_t* __restrict__ bits, int64_t N, int64_t words, const uint32_t* __restrict__ visible,
                               int min_num_poses, int invert, int64_t* __restrict__ mask, int32_t* __restrict__ count) {
    const int64_t v = (int64_t)blockIdx.x * OB + threadIdx.x;
    if (v >= N) return;
    const uint32_t* row = bits + v * words;
    const uint32_t* vis = visible + (int64_t)blockIdx.y * words;
    int c = 0;
    for (int64_t w = 0; w < words; ++w) c += __popc(row[w] & vis[w]);
    const int64_t o = (int64_t)blockIdx.y * N + v;
    if (mask != nullptr) mask[o] = (int64_t)((c >= min_num_poses ? 1 : 0) ^ (invert ? 1 : 0));
    if (count != nullptr) count[o] = c;
}

}  // namespace

extern "C" size_t stin_observe_workspace_bytes(int64_t N, int64_t F, int S, int batch) {
    if (N < 0 || F < 0 || S < 1 || S > STIN_OBSERVE_MAX_SIZE || batch < 1 || batch > STIN_OBSERVE_MAX_BATCH) return 0;
    return observe_layout(N, F, S, batch).total;
}

extern "C" int stin_observe_poses_f64(const double* vertices, int64_t N, const int64_t* faces, int64_t F, const double* RT,
                                      const uint8_t* valid, int64_t P, double sx, double sy, int S, double z_near, int batch,
                                      int64_t large_box, uint32_t* bits, int64_t words, int32_t* status, void* workspace,
                                      size_t workspace_bytes, stin_stream_t stream_) {
    STIN_REQUIRE(N >= 0 && F >= 0 && P >= 0 && N < (int64_t)INT32_MAX && F < (int64_t)INT32_MAX, STIN_E_SIZE);
    STIN_REQUIRE(S >= 1 && S <= STIN_OBSERVE_MAX_SIZE && batch >= 1 && batch <= STIN_OBSERVE_MAX_BATCH, STIN_E_SIZE);
    STIN_REQUIRE(words >= (P + 31) / 32 && z_near > 0.0, STIN_E_SIZE);
    STIN_REQUIRE(status != nullptr && (N == 0 || vertices) && (N == 0 || words == 0 || bits), STIN_E_NULL);
    STIN_REQUIRE((F == 0 || faces) && (P == 0 || (RT && valid)), STIN_E_NULL);
    STIN_REQUIRE(workspace != nullptr && workspace_bytes >= stin_observe_workspace_bytes(N, F, S, batch), STIN_E_WORKSPACE);
    hipStream_t stream = (hipStream_t)stream_;
    stin_clear_stale_error();
    RasterCall c = {vertices, N, F, RT, valid, {STIN_RASTER_SQUARE, {sx, sy, 0.5 * (double)S, 0.0}}, S, S, z_near,
                    large_box > 0 ? large_box : STIN_OBSERVE_LARGE_BOX, LARGE_GRID, status};
    stin_raster_bind(c, observe_layout(N, F, S, batch), workspace);
    (void)hipMemsetAsync(status, 0, 4, stream);
    if (N > 0 && words > 0) (void)hipMemsetAsync(bits, 0, (size_t)N * (size_t)words * 4, stream);
    if (N == 0 || F == 0 || P == 0) return stin_launch_status();
    const int64_t S2 = (int64_t)S * S;
    stin_raster_faces(c, faces, stream);
    for (int64_t p0 = 0; p0 < P; p0 += batch) {
        const unsigned nb = (unsigned)(P - p0 < batch ? P - p0 : batch);
        stin_raster_batch(c, p0, nb, (int64_t)nb * S2, 0, STIN_RASTER_ALL_STAGES, stream);
        hipLaunchKernelGGL(k_observe_resolve, dim3((unsigned)((S2 + OB - 1) / OB), nb), dim3(OB), 0, stream, c.keys, c.f32, S2, p0, bits,
                           words);
    }
    return stin_launch_status();
}

extern "C" int stin_observe_mask_u32(const uint32_t* bits, int64_t N, int64_t words, const uint32_t* visible_words, int M,
                                     int min_num_poses, int invert, int64_t* mask, int32_t* count, stin_stream_t stream_) {
    STIN_REQUIRE(N >= 0 && words >= 0 && M >= 0 && M <= 65535, STIN_E_SIZE);
    STIN_REQUIRE(mask != nullptr || count != nullptr, STIN_E_NULL);
    if (N == 0 || M == 0) return STIN_OK;
    STIN_REQUIRE(words == 0 || (bits && visible_words), STIN_E_NULL);
    stin_clear_stale_error();
    hipLaunchKernelGGL(k_observe_mask, dim3((unsigned)((N + OB - 1) / OB), (unsigned)M), dim3(OB), 0, (hipStream_t)stream_, bits, N, words,
                       visible_words, min_num_poses, invert, mask, count);
    return stin_launch_status();
}
