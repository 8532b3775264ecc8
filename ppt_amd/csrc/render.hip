// render.hip -- what notebook/show_balls.py shows of a part-segmentation model, on the device (ppt_amd/viz.py): the per-point
// predictions (show_balls.py:256-262) and the shaded-ball pictures of ground truth and prediction (its render_ball call), for
// whole validation batches and several views at once.
//
//   partseg_predict_kernel  one thread per point: the first arg-max over the part range of the cloud's category, the rule of
//                           partseg_metrics_kernel (metrics.hip), written out per point instead of counted.
//   render_range_kernel     one workgroup per geometry: min and max depth over all of its points (the brightness range).
//   render_balls_kernel     one workgroup per 64 x 64 screen tile of one geometry.  The tile's depth test is a buffer of 64-bit keys
//                           in LDS; the workgroup walks the geometry's points 256 at a time, keeps those whose ball's bounding box
//                           meets the tile in an LDS list, and each wave splats one listed point at a time, lane = pattern entry,
//                           with ds_max_u64.  A maximum does not depend on the order of its operands, so the winners -- and every
//                           byte of the pictures -- are the same on every run; there are no global atomics.  Visibility does not
//                           depend on colour: it is resolved once, then the tile of each of the K pictures is shaded and written
//                           once, 48 bytes (16 pixels) per thread.
// The key: (depth offer z2, biased to unsigned) << 32 | (0xFFFF - point) << 16 | pattern entry.  The larger depth wins, equal
// depths go to the LOWER point index -- what a sequential loop over the points with a strict `<` depth test leaves -- and for one
// pixel and one point the pattern entry is fixed, so the low 16 bits never decide: the order is that of
// (z2 biased) << 32 | (0xFFFFFFFF - point), and the shading pass finds the entry's shade without reading the point again.
// All pixel arithmetic is in double, uncontracted (-ffp-contract=off), in the order include/ppt_hip.h states.
#include "ppt_common.h"

#define RB_TILE 64                         // screen tile: RB_TILE x RB_TILE pixels per workgroup
#define RB_STRIDE (RB_TILE + 2)            // keys per tile row in LDS: 4 dwords of padding per row (see the shading pass)
#define RB_THREADS 256
#define RB_WAVES (RB_THREADS / PPT_WAVE)
#define RB_UNIT 16                         // pixels per thread in the shading pass: 48 bytes, three 16-byte stores
#define RB_MAX_RADIUS 16
#define RB_MAX_SIDE (2 * RB_MAX_RADIUS - 1)
#define RB_PASSES ((RB_MAX_SIDE * RB_MAX_SIDE + PPT_WAVE - 1) / PPT_WAVE)      // pattern entries per lane
#define RB_MAX_IMAGE 4096
#define RB_MAX_POINTS 65536

__global__ __launch_bounds__(256) void partseg_predict_kernel(const float *__restrict__ logits, const int64_t *__restrict__ anchor,
                                                              int N, int P, const int32_t *__restrict__ part_start,
                                                              const int32_t *__restrict__ part_count, int32_t *__restrict__ pred)
{
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    // the tables are device memory the host entry cannot look into: clamp what they say so that no index leaves the row
    const int64_t a = anchor[b];
    const bool bad = a < 0 || a >= (int64_t)P;
    int start = bad ? 0 : part_start[a];
    int count = bad ? 0 : part_count[a];
    start = max(0, min(start, P));
    count = max(0, min(count, P - start));
    int best_c = -1;
    if (count > 0) {                                       // the first maximum wins (metrics.hip: the same loop)
        const float *x = logits + ((size_t)b * N + n) * P;
        float best = x[start];
        best_c = start;
        for (int c = start + 1; c < start + count; c++) {
            const float v = x[c];
            if (v > best) { best = v; best_c = c; }
        }
    }
    pred[(size_t)b * N + n] = best_c;
}

__global__ __launch_bounds__(RB_THREADS) void render_range_kernel(const int32_t *__restrict__ ixyz, int n, int32_t *__restrict__ range)
{
    __shared__ int lo_s[RB_WAVES], hi_s[RB_WAVES];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int32_t *pts = ixyz + (size_t)g * n * 3;
    int lo = INT32_MAX, hi = INT32_MIN;
    for (int i = tid; i < n; i += RB_THREADS) {
        const int z = pts[3 * (size_t)i + 2];
        lo = min(lo, z);
        hi = max(hi, z);
    }
    for (int o = 32; o; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o));
        hi = max(hi, __shfl_xor(hi, o));
    }
    if ((tid & 63) == 0) { lo_s[tid >> 6] = lo; hi_s[tid >> 6] = hi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < RB_WAVES; w++) { lo = min(lo, lo_s[w]); hi = max(hi, hi_s[w]); }
        range[2 * g] = lo;
        range[2 * g + 1] = hi;
    }
}

struct rb_background { unsigned char c[3]; };
struct rb_point { int x, y, z; };                          // 12 bytes, 4-byte aligned: one dwordx3 load
typedef float rb_f32x3 __attribute__((ext_vector_type(3)));
typedef rb_f32x3 rb_rgb __attribute__((aligned(4)));       // a colour: likewise

// pattern [side * side][2] double, side = 2 r - 1, entry (dx + r - 1) * side + (dy + r - 1): dz = sqrt(r^2 - dx^2 - dy^2) and the
// shade dz / r where dx^2 + dy^2 < r^2, dz < 0 elsewhere.  div_magic: e / side == (e * div_magic) >> 16 for every e < side * side.
__global__ __launch_bounds__(RB_THREADS) void render_balls_kernel(const int32_t *__restrict__ ixyz, const float *__restrict__ colors,
                                                                  const double *__restrict__ pattern,
                                                                  const int32_t *__restrict__ range, rb_background bg, int K, int n,
                                                                  int H, int W, int r, unsigned div_magic, int tiles_c,
                                                                  int tiles_per_image, int wide, unsigned char *__restrict__ out)
{
    __shared__ unsigned long long tile[RB_TILE * RB_STRIDE];
    __shared__ int4 list[RB_THREADS];
    __shared__ int list_n[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = blockIdx.x / tiles_per_image, t = blockIdx.x - g * tiles_per_image;
    const int row0 = (t / tiles_c) * RB_TILE, col0 = (t % tiles_c) * RB_TILE;
    const int side = 2 * r - 1, entries = side * side, reach = r - 1;
    const int32_t *pts = ixyz + (size_t)g * n * 3;

    for (int i = tid; i < RB_TILE * RB_STRIDE; i += RB_THREADS) tile[i] = 0ull;        // 0: nobody reached the pixel
    if (tid < 2) list_n[tid] = 0;
    // A lane splats the same pattern entries, lane + 64 j, of every point: their depths and offsets stay in registers
    double dz_r[RB_PASSES];
    int off_r[RB_PASSES];                                  // dx << 16 | (dy & 0xFFFF)
#pragma unroll
    for (int j = 0; j < RB_PASSES; j++) {
        const int e = lane + PPT_WAVE * j;
        const int q = (int)(((unsigned)e * div_magic) >> 16);
        dz_r[j] = e < entries ? pattern[2 * e] : -1.0;
        off_r[j] = (int)(((unsigned)(q - reach) << 16) | ((unsigned)(e - q * side - reach) & 0xFFFFu));
    }
    __syncthreads();

    // ---- visibility: the points in chunks of RB_THREADS; list_n[] alternates so that a count is cleared a chunk after its use --
    // The next chunk's point is loaded before this chunk is splatted: its latency passes under the LDS work.
    rb_point next = {0, 0, 0};
    if (tid < n) next = *reinterpret_cast<const rb_point *>(pts + 3 * (size_t)tid);
    for (int base = 0, chunk = 0; base < n; base += RB_THREADS, chunk++) {
        const int slot_n = chunk & 1;
        const int i = base + tid;
        const int x = next.x, y = next.y, z = next.z;
        if (i + RB_THREADS < n) next = *reinterpret_cast<const rb_point *>(pts + 3 * ((size_t)i + RB_THREADS));
        if (i < n) {
            // the ball's bounding box against the tile (no x - row0 before the test: x is any int32)
            if (x >= row0 - reach && x <= row0 + RB_TILE - 1 + reach && y >= col0 - reach && y <= col0 + RB_TILE - 1 + reach) {
                const int slot = atomicAdd(&list_n[slot_n], 1);                         // (the order of the list decides nothing)
                list[slot] = make_int4(x - row0, y - col0, z, i);
            }
        }
        __syncthreads();
        const int listed = list_n[slot_n];
        if (tid == 0) list_n[slot_n ^ 1] = 0;
        for (int j = wave; j < listed; j += RB_WAVES) {
            const int4 p = list[j];
            const unsigned low = (unsigned)(0xFFFF - p.w) << 16;
            const double z = (double)p.z;
#pragma unroll
            for (int k = 0; k < RB_PASSES; k++) {
                if (PPT_WAVE * k < entries) {                                           // wave-uniform
                    const double dz = dz_r[k];
                    const int px = p.x + (off_r[k] >> 16), py = p.y + (int)(short)off_r[k];
                    if (dz >= 0.0 && px >= 0 && px < RB_TILE && py >= 0 && py < RB_TILE) {
                        const int z2 = (int)(z + dz);                                   // truncates toward zero
                        const unsigned long long key = ((unsigned long long)((unsigned)z2 ^ 0x80000000u) << 32)
                                                       | (low | (unsigned)(lane + PPT_WAVE * k));
                        atomicMax(&tile[px * RB_STRIDE + py], key);
                    }
                }
            }
        }
        __syncthreads();
    }

    // ---- shading: thread -> 16 consecutive pixels of one tile row.  The four threads of a row read keys 128 bytes apart and the
    // rows of a 32-lane group are 4 dwords apart (RB_STRIDE): two lanes per bank instead of sixteen ------------------------------
    const int row = tid >> 2, gx = row0 + row, gy0 = col0 + (tid & 3) * RB_UNIT;
    if (gx >= H || gy0 >= W) return;
    const double zmin = (double)range[2 * g] - (double)r, zmax = (double)range[2 * g + 1] + (double)r;
    const double zspan = zmax - zmin;
    int who[RB_UNIT];                                      // the winning point, -1: background
    double shade[RB_UNIT], light[RB_UNIT];
#pragma unroll
    for (int p = 0; p < RB_UNIT; p++) {
        const unsigned long long key = tile[row * RB_STRIDE + (tid & 3) * RB_UNIT + p];
        const unsigned low = (unsigned)key;
        const int z2 = (int)((unsigned)(key >> 32) ^ 0x80000000u);
        who[p] = key ? 0xFFFF - (int)(low >> 16) : -1;
        const double s = pattern[2 * (key ? (low & 0xFFFFu) : 0u) + 1];                // (loaded for every pixel, then selected)
        shade[p] = key ? s : 0.0;
        const double v = ((double)z2 - zmin) / zspan * 0.7 + 0.3;
        light[p] = v < 1.0 ? v : 1.0;
    }
    for (int k = 0; k < K; k++) {
        // (n = 0: there are no colours, and the dropped load below still needs 12 readable bytes -- the pattern has them)
        const float *col = n ? colors + ((size_t)g * K + k) * n * 3 : reinterpret_cast<const float *>(pattern);
        uint32_t w[3 * RB_UNIT / 4];
#pragma unroll
        for (int j = 0; j < 3 * RB_UNIT / 4; j++) w[j] = 0u;
#pragma unroll
        for (int p = 0; p < RB_UNIT; p++) {
            // (a background pixel reads point 0's colour and drops it: a load no branch waits for)
            const rb_f32x3 rgb = *reinterpret_cast<const rb_rgb *>(col + 3 * (size_t)max(who[p], 0));
#pragma unroll
            for (int c = 0; c < 3; c++) {
                // computed for every pixel and selected afterwards: no branch per byte (a background pixel's shade is 0)
                const unsigned lit = (unsigned)(shade[p] * (double)rgb[c] * light[p]) & 0xFFu;
                const unsigned v = who[p] >= 0 ? lit : (unsigned)bg.c[c];
                w[(3 * p + c) >> 2] |= v << (8 * ((3 * p + c) & 3));
            }
        }
        unsigned char *dst = out + ((((size_t)g * K + k) * H + gx) * W + gy0) * 3;
        if (wide) {                                        // W % 16 == 0 and an aligned image: the unit is whole and 16-byte aligned
#pragma unroll
            for (int j = 0; j < 3; j++) ppt_store16_stream(dst + 16 * j, make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]));
        } else {
#pragma unroll
            for (int p = 0; p < RB_UNIT; p++) {
                if (gy0 + p < W) {
#pragma unroll
                    for (int c = 0; c < 3; c++) dst[3 * p + c] = (unsigned char)(w[(3 * p + c) >> 2] >> (8 * ((3 * p + c) & 3)));
                }
            }
        }
    }
}

extern "C" int ppt_partseg_predict(const float *logits, const int64_t *anchor, int B, int N, int P, const int32_t *part_start,
                                   const int32_t *part_count, int32_t *pred, void *stream)
{
    if (!logits || !anchor || !part_start || !part_count || !pred || B <= 0 || N <= 0 || P <= 0) return PPT_EINVAL;
    if (((uintptr_t)logits & 3) || ((uintptr_t)pred & 3)) return PPT_EINVAL;
    if (P > 64) return PPT_EUNSUPPORTED;
    if (B > 65535) return PPT_EINVAL;
    hipLaunchKernelGGL(partseg_predict_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)B), dim3(256), 0, ppt_stream(stream), logits,
                       anchor, N, P, part_start, part_count, pred);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}

static inline bool rb_supported(int G, int n, int H, int W, int radius)
{
    return G > 0 && n >= 0 && H > 0 && W > 0 && radius <= RB_MAX_RADIUS && H <= RB_MAX_IMAGE && W <= RB_MAX_IMAGE && n <= RB_MAX_POINTS;
}

extern "C" size_t ppt_render_balls_workspace_bytes(int G, int n, int H, int W, int radius)
{
    if (!rb_supported(G, n, H, W, radius)) return 0;
    return ((size_t)G * 2 * sizeof(int32_t) + 255) & ~(size_t)255;                     // the depth range of every geometry
}

extern "C" int ppt_render_balls(const int32_t *ixyz, const float *colors, const double *pattern, const unsigned char *background,
                                int radius, int G, int K, int n, int H, int W, unsigned char *out, void *workspace,
                                size_t workspace_bytes, void *stream)
{
    if (!pattern || !background || !out || !workspace || G <= 0 || K <= 0 || n < 0 || H <= 0 || W <= 0) return PPT_EINVAL;
    if (n > 0 && (!ixyz || !colors)) return PPT_EINVAL;
    if (((uintptr_t)ixyz & 3) || ((uintptr_t)colors & 3) || ((uintptr_t)pattern & 7) || ((uintptr_t)workspace & 255)) return PPT_EINVAL;
    if (!rb_supported(G, n, H, W, radius)) return PPT_EUNSUPPORTED;
    if (workspace_bytes < ppt_render_balls_workspace_bytes(G, n, H, W, radius)) return PPT_EINVAL;
    const int r = radius < 1 ? 1 : radius, side = 2 * r - 1;
    const int tiles_c = (W + RB_TILE - 1) / RB_TILE, tiles_per_image = tiles_c * ((H + RB_TILE - 1) / RB_TILE);
    if ((int64_t)G * tiles_per_image > 0x7fffffffLL) return PPT_EINVAL;
    rb_background bg;
    for (int c = 0; c < 3; c++) bg.c[c] = background[c];
    int32_t *range = reinterpret_cast<int32_t *>(workspace);
    if (n > 0) {
        hipLaunchKernelGGL(render_range_kernel, dim3((unsigned)G), dim3(RB_THREADS), 0, ppt_stream(stream), ixyz, n, range);
        PPT_CHECK_LAUNCH();
    }
    const int wide = (W % 16 == 0) && !((uintptr_t)out & 15);
    hipLaunchKernelGGL(render_balls_kernel, dim3((unsigned)(G * tiles_per_image)), dim3(RB_THREADS), 0, ppt_stream(stream), ixyz,
                       colors, pattern, range, bg, K, n, H, W, r, 65536u / (unsigned)side + 1u, tiles_c, tiles_per_image, wide, out);
    PPT_CHECK_LAUNCH();
    return PPT_OK;
}
