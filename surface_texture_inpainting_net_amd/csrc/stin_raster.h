// The depth-key rasteriser under the observer masks (stin_observe.hip) and the result views (stin_render.hip): host declarations;
// the kernels and what each stage does are in stin_raster.hip.
#pragma once
#include "stin_common.h"

constexpr unsigned long long STIN_RASTER_NO_FACE = ~0ull;                 // a key nobody has lowered
// the stage bits are render's public ones (stin_hip.h); a resolve pass is its caller's
constexpr int STIN_RASTER_ALL_STAGES = STIN_RENDER_STAGE_CLEAR | STIN_RENDER_STAGE_TRANSFORM | STIN_RENDER_STAGE_RASTER | STIN_RENDER_STAGE_LARGE;

// Byte offsets of the rasteriser's share of a workspace (each region 256-byte aligned) and the entries of the large-face queue.
struct RasterLayout {
    size_t faces, coords, keys, queue, ctl, total;
    unsigned queue_cap;
};
// key_count: the keys of one batch, with whatever slack the caller's resolve pass wants behind them
RasterLayout stin_raster_layout(int64_t N, int64_t F, int batch, size_t key_count);

// (xv, yv, zv) -> screen.  SQUARE, p = (sx, sy, half): X = (sx xv / zv + 1.0) half - 0.5 (the observers' contract);
// PINHOLE, p = (fx, fy, cx, cy): X = fx xv / zv + cx (render's); Y likewise.  Two expressions, not one: the oracles compare bits.
enum RasterScreen { STIN_RASTER_SQUARE, STIN_RASTER_PINHOLE };
struct RasterProjection {
    RasterScreen screen;
    double p[4];
};

// What stays the same over the batches of a call.
struct RasterCall {
    const double* vertices;            // [N][3]
    int64_t N, F;
    const double* RT;                  // [P][12]
    const uint8_t* valid;              // [P]
    RasterProjection proj;
    int H, W;
    double z_near;
    int64_t large_box;                 // a clamped box of more centres goes to the wavefront kernel
    int large_grid;                    // workgroups of that kernel (4 waves each, entries strided)
    int32_t* status;                   // device word: bit 1 a bad index, bit 2 a face went through the large-face kernel
    int32_t* f32;                      // the layout's regions (stin_raster_bind)
    double* coords;
    unsigned long long* keys;
    unsigned long long* queue;
    unsigned queue_cap;
    unsigned* qcount;
};

inline void stin_raster_bind(RasterCall& c, const RasterLayout& L, void* workspace) {
    char* w = (char*)workspace;
    c.f32 = (int32_t*)(w + L.faces);
    c.coords = (double*)(w + L.coords);
    c.keys = (unsigned long long*)(w + L.keys);
    c.queue = (unsigned long long*)(w + L.queue);
    c.queue_cap = L.queue_cap;
    c.qcount = (unsigned*)(w + L.ctl);
}
// faces int64 -> c.f32, once per call
void stin_raster_faces(const RasterCall& c, const int64_t* faces, hipStream_t stream);
// One batch, poses [p0, p0 + nb): the stages of `stages`, in order.  clear: the first clear_keys keys of c.keys (rounded up to a pair:
// the layout's padding holds the extra one) and the queue counter; pose b's keys are c.keys + key_offset + b H W.
void stin_raster_batch(const RasterCall& c, int64_t p0, unsigned nb, int64_t clear_keys, int64_t key_offset, int stages, hipStream_t stream);
