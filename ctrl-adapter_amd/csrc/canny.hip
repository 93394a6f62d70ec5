// Canny condition extraction on the GPU: model/ctrl_helper.py:171-179, `cv2.Canny(np.array(img), 100, 200)` and the three-fold
// channel replication that follows it, for a whole clip at once.  OpenCV's Canny (apertureSize 3, L2gradient false) is integer
// arithmetic from the first Sobel tap to the last hysteresis step, so the result is OpenCV's bit for bit (tests/canny_ref.py
// restates it; tests/golden/canny/ holds cv2's own outputs).  Three kernels:
//   canny_map_kernel   uint8 [N][H][W][C] -> one byte per pixel: 0 none, 1 weak, 2 strong candidate
//   canny_hyst_kernel  one pass of "promote 1 -> 2 next to a 2", tile by tile, until a pass promotes nothing
//   canny_finish_kernel map -> 0 / 255 as [N][H][W] or [N][H][W][3]
// One tile (64 x 64 pixels: 256 threads in the map kernel, one wave in the hysteresis) serves the first two; ctrl_canny_launch_shape
// reports it.
//
// Traffic per pixel: the map kernel reads C bytes (+ 13 % halo) and writes 1; a hysteresis pass reads 1 (+ 6 % halo) and writes 1
// only from threads whose 16-pixel strip changed; the finish reads 1 and writes 1 or 3.  Every global access that can be is a dword:
//   * source tile: the staged row segment is copied as the ALIGNED dwords that cover it, into an LDS row that keeps the global
//     address' phase (byte g of the segment lands at an LDS offset = g mod 4), so no byte is ever shifted; a dword is loaded
//     whole when it lies inside the caller's buffer [src, src + N*H*W*C) and byte by byte otherwise (the first / last dword of a buffer
//     that does not start or end on a dword, or W*C not a multiple of 4 at the buffer's end)
//   * map and output: dword per 4 pixels where the row address is dword-aligned and the 4 pixels are inside the row, bytes otherwise.
#include "ops.h"
#include <algorithm>
#include <cmath>
#include <mutex>

namespace {

constexpr int TH = 64, TW = 64, NT = 256;
// OpenCV's TG22 = (int)(0.4142135623730950488016887242097 * (1 << 15) + 0.5) (canny.cpp, CANNY_SHIFT 15).  The golden images do not
// tell 13573 from 13572 (tests/test_canny_host.py plants that error and finds no pixel moved): the constant is OpenCV's source's.
constexpr int kTan22 = 13573;
constexpr int kShift = 15;

constexpr int kMaxBatch = 16;             // hysteresis passes per readback, at most (CTRL_CANNY_BATCH)
constexpr int kFlagBytes = 256;           // the flag block at the start of the workspace: kMaxBatch words, padded

// ---- map ----------------------------------------------------------------------------------------------------------------
// stage (TH + 4) x (TW + 4) source pixels (Sobel needs 1 beyond the magnitudes, which are needed 1 beyond the tile); the replicate border is
// applied while staging, so the Sobel never looks at coordinates again.
template <int C> struct MapGeom {
    static constexpr int PH = TH + 4, PW = TW + 4;
    static constexpr int RS = ((PW * C + 6 + 3) / 4) * 4;        // LDS row: the segment + 3 bytes of phase + the last dword's tail
    static constexpr int DW = RS / 4;                           // (53 / 19 dwords: odd, rows walk the banks)
    static constexpr int MH = TH + 2, MW = TW + 2, MS = MW + 1;
};

template <int C>
__global__ __launch_bounds__(NT) void canny_map_kernel(const unsigned char* __restrict__ src, size_t total_bytes, int H, int W,
                                                       int tiles_x, int tiles_y, int low, int high, unsigned char* __restrict__ map) {
    typedef MapGeom<C> G;
    __shared__ __attribute__((aligned(16))) unsigned char px[G::PH * G::RS];
    __shared__ unsigned int mg[G::MH * G::MS];            // m | |dx| << 11 | ((dx ^ dy) < 0) << 21 of the chosen channel; 0 outside the image
    __shared__ unsigned char phs[G::PH];                  // phase (global address & 3) of every staged row's column 0
    const int t = threadIdx.x;
    int b = blockIdx.x;
    const int tx = b % tiles_x; b /= tiles_x;
    const int ty = b % tiles_y;
    const int n = b / tiles_y;
    const int y0 = ty * TH, x0 = tx * TW;
    const unsigned char* img = src + (size_t)n * H * W * C;
    const uintptr_t lo_addr = (uintptr_t)src, hi_addr = (uintptr_t)src + total_bytes;
    const int cs = max(x0 - 2, 0), ce = min(x0 + G::PW - 2, W);          // staged in-image columns [cs, ce)

    for (int i = t; i < G::PH * G::DW; i += NT) {
        const int r = i / G::DW, k = i - r * G::DW;
        const int y = min(max(y0 - 2 + r, 0), H - 1);                    // replicate rows: the clamped row is staged again
        const unsigned char* rowp = img + (size_t)y * W * C;
        const intptr_t v0 = (intptr_t)rowp + (intptr_t)(x0 - 2) * C;     // address column 0 of the staged row has (or would have)
        const int ph = (int)(v0 & 3);
        if (k == 0) phs[r] = (unsigned char)ph;
        const uintptr_t g0 = (uintptr_t)(rowp + (size_t)cs * C), g1 = (uintptr_t)(rowp + (size_t)ce * C);
        const uintptr_t ga = (g0 & ~(uintptr_t)3) + 4u * (unsigned)k;
        if (ga >= g1) continue;
        const int L = r * G::RS + ph + (int)((intptr_t)ga - v0);          // a multiple of 4 inside row r (see MapGeom::RS)
        if (ga >= lo_addr && ga + 4 <= hi_addr) {
            *(unsigned int*)(px + L) = *(const unsigned int*)ga;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ga + j >= g0 && ga + j < g1) px[L + j] = *(const unsigned char*)(ga + j);
        }
    }
    __syncthreads();
    if (x0 == 0 || x0 + G::PW - 2 > W) {                                  // replicate columns (the copy above may have left neighbours' bytes there)
        for (int i = t; i < G::PH * G::PW; i += NT) {
            const int r = i / G::PW, c = i - r * G::PW;
            const int x = x0 - 2 + c;
            if (x >= 0 && x < W) continue;
            const int cc = min(max(x, 0), W - 1) - x0 + 2;
            unsigned char* row = px + r * G::RS + phs[r];
#pragma unroll
            for (int ch = 0; ch < C; ++ch) row[c * C + ch] = row[cc * C + ch];
        }
        __syncthreads();
    }

    for (int i = t; i < G::MH * G::MW; i += NT) {
        const int r = i / G::MW, c = i - r * G::MW;
        const int y = y0 - 1 + r, x = x0 - 1 + c;
        unsigned int word = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const unsigned char* ra = px + r * G::RS + phs[r] + c * C;              // staged row r = image row y - 1, staged column c = x - 1
            const unsigned char* rb = px + (r + 1) * G::RS + phs[r + 1] + c * C;
            const unsigned char* rc = px + (r + 2) * G::RS + phs[r + 2] + c * C;
            int best = -1;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const int a0 = ra[ch], a1 = ra[C + ch], a2 = ra[2 * C + ch];
                const int b0 = rb[ch], b2 = rb[2 * C + ch];
                const int c0 = rc[ch], c1 = rc[C + ch], c2 = rc[2 * C + ch];
                const int dx = (a2 + 2 * b2 + c2) - (a0 + 2 * b0 + c0);
                const int dy = (c0 + 2 * c1 + c2) - (a0 + 2 * a1 + a2);
                const int m = abs(dx) + abs(dy);
                if (m > best) {                                                     // strict: the FIRST channel with the maximal magnitude
                    best = m;
                    word = (unsigned)m | ((unsigned)abs(dx) << 11) | (((dx ^ dy) < 0) ? (1u << 21) : 0u);
                }
            }
        }
        mg[r * G::MS + c] = word;
    }
    __syncthreads();

    unsigned char* mimg = map + (size_t)n * H * W;
    for (int i = t; i < TH * (TW / 4); i += NT) {
        const int r = i / (TW / 4), c4 = (i - r * (TW / 4)) * 4;
        const int y = y0 + r, xb = x0 + c4;
        if (y >= H || xb >= W) continue;
        unsigned int packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned int* q = mg + (r + 1) * G::MS + c4 + j + 1;
            const unsigned int w = q[0];
            const int m = (int)(w & 2047u);
            unsigned int v = 0;
            if (xb + j < W && m > low) {
                const int ax = (int)((w >> 11) & 1023u), ay = m - ax;
                const int yy = ay << kShift, t22 = ax * kTan22, t67 = t22 + (ax << (kShift + 1));
                bool cand;
                if (yy < t22) {
                    cand = m > (int)(q[-1] & 2047u) && m >= (int)(q[1] & 2047u);
                } else if (yy > t67) {
                    cand = m > (int)(q[-G::MS] & 2047u) && m >= (int)(q[G::MS] & 2047u);
                } else {
                    const int s = (w >> 21) ? -1 : 1;
                    cand = m > (int)(q[-G::MS - s] & 2047u) && m > (int)(q[G::MS + s] & 2047u);
                }
                if (cand) v = m > high ? 2u : 1u;
            }
            packed |= v << (8 * j);
        }
        unsigned char* o = mimg + (size_t)y * W + xb;
        if (xb + 3 < W && ((uintptr_t)o & 3) == 0) {
            *(unsigned int*)o = packed;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (xb + j < W) o[j] = (unsigned char)(packed >> (8 * j));
        }
    }
}

// ---- hysteresis -------------------------------------------------------------------------------------------------------------
// The result -- every weak pixel 8-connected to a strong one through candidates becomes strong -- is the least fixpoint of "a 1 with a 2
// among its 8 neighbours becomes 2".  Promotions only ever turn 1 into 2 and only next to a 2 that the fixpoint also holds, so ANY
// order of applying the rule, with any mixture of old and new neighbour values, stays below the fixpoint and reaches it once no rule
// applies: the bytes at the end do not depend on the schedule.
//   * Inside a tile there is no race at all: ONE wave owns a 64 x 64 tile, lane r holds row r as two 64-bit masks (weak, strong) in
//     registers, and a sweep is a handful of shifts: the strong bits of the rows above and below arrive by lane shuffles, "next to a
//     strong pixel" is v | v << 1 | v >> 1, and a promotion runs along its whole run of weak pixels in the same sweep (six doubling steps
//     each way).  The wave sweeps until no lane promoted (__any).  A winding edge needs dozens of sweeps, so a sweep has to be
//     cheap: with the tile kept as bytes in LDS the pass loop measured 7 times slower.
//   * Across tiles, a wave's halo is its neighbours' interior as it was at SOME time during this pass (a neighbour may store in the same
//     pass, and this CU's L1 may hold the older line).  A stale halo byte is an old 1 where a 2 now stands; the promotion it would have
//     caused is not lost, only postponed: the neighbour that stored raised the pass flag, so another pass follows, and a kernel boundary
//     makes every store of this pass visible to it.  A pass in which no workgroup raised the flag read only settled bytes (nothing was stored
//     in it) and found no rule to apply anywhere: the fixpoint.
// A workgroup stores only rows of its own interior, so no byte has two writers.
static_assert(TH == 64 && TW == 64, "the hysteresis kernel keeps a tile row in a 64-bit mask and a tile in one wave");
typedef unsigned long long u64;

__global__ __launch_bounds__(64) void canny_hyst_kernel(unsigned char* map, int H, int W, int tiles_x, int tiles_y, int* flag) {
    const int lane = threadIdx.x;
    int b = blockIdx.x;
    const int tx = b % tiles_x; b /= tiles_x;
    const int ty = b % tiles_y;
    const int n = b / tiles_y;
    const int y0 = ty * TH, x0 = tx * TW;
    unsigned char* mimg = map + (size_t)n * H * W;
    auto strong_at = [&](int y, int x) -> bool { return y >= 0 && y < H && x >= 0 && x < W && mimg[(size_t)y * W + x] == 2; };

    // lane r: row y0 + r of the tile; pixels outside the image are 0
    const int y = y0 + lane;
    u64 wk = 0, st = 0;
    if (y < H) {
#pragma unroll
        for (int q = 0; q < TW / 4; ++q) {
            const int xb = x0 + 4 * q;
            if (xb >= W) break;
            const unsigned char* p = mimg + (size_t)y * W + xb;
            unsigned int v = 0;
            if (xb + 3 < W && ((uintptr_t)p & 3) == 0) {
                v = *(const unsigned int*)p;
            } else {
                for (int j = 0; j < 4; ++j)
                    if (xb + j < W) v |= (unsigned int)p[j] << (8 * j);
            }
            // a byte is 0, 1 or 2: bit 0 = weak, bit 1 = strong; the multiplication gathers the four bits into the top nibble
            wk |= (u64)(((v & 0x01010101u) * 0x10204080u) >> 28) << (4 * q);
            st |= (u64)((((v >> 1) & 0x01010101u) * 0x10204080u) >> 28) << (4 * q);
        }
    }
    // the halo: only its strong pixels matter, and they do not change during the pass
    const u64 top = __ballot(strong_at(y0 - 1, x0 + lane)), bot = __ballot(strong_at(y0 + TH, x0 + lane));
    const u64 corner = __ballot(lane < 4 && strong_at(lane < 2 ? y0 - 1 : y0 + TH, (lane & 1) ? x0 + TW : x0 - 1));   // tl, tr, bl, br
    const bool hl = strong_at(y, x0 - 1), hr = strong_at(y, x0 + TW);
    const u64 side = __ballot(hl), side_r = __ballot(hr);
    // strong pixels in columns -1 and TW of the rows lane - 1 .. lane + 1: they touch this row's first and last pixel
    bool nl = hl, nr = hr;
    nl |= lane == 0 ? (corner & 1) != 0 : ((side >> (lane - 1)) & 1) != 0;
    nr |= lane == 0 ? (corner & 2) != 0 : ((side_r >> (lane - 1)) & 1) != 0;
    nl |= lane == 63 ? (corner & 4) != 0 : ((side >> (lane + 1)) & 1) != 0;
    nr |= lane == 63 ? (corner & 8) != 0 : ((side_r >> (lane + 1)) & 1) != 0;
    const u64 edge = (nl ? 1ull : 0ull) | (nr ? 1ull << 63 : 0ull);

    bool mine_changed = false, tile_changed = false;
    for (;;) {
        u64 up = __shfl_up(st, 1), dn = __shfl_down(st, 1);
        if (lane == 0) up = top;
        if (lane == 63) dn = bot;
        const u64 v = up | st | dn;
        u64 s = wk & (v | (v << 1) | (v >> 1) | edge);
        if (s) {
            // run the promotion along the row: occluded fill through the weak pixels, to the left and to the right
            u64 r = s, m = wk, l = s;
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) { r |= m & (r << k); m &= m << k; }
            m = wk;
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) { l |= m & (l >> k); m &= m >> k; }
            s = r | l;
            st |= s;
            wk &= ~s;
            mine_changed = true;
        }
        if (!__any(s != 0)) break;
        tile_changed = true;
    }
    if (mine_changed) {                                                   // a changed pixel is inside the image: so is its row
#pragma unroll
        for (int q = 0; q < TW / 4; ++q) {
            const int xb = x0 + 4 * q;
            if (xb >= W) break;
            // four mask bits back to four bytes: bit i of the nibble to bit 8 i
            const unsigned int w4 = (unsigned int)(wk >> (4 * q)) & 15u, s4 = (unsigned int)(st >> (4 * q)) & 15u;
            const unsigned int v = ((w4 * 0x00204081u) & 0x01010101u) | (((s4 * 0x00204081u) & 0x01010101u) << 1);
            unsigned char* o = mimg + (size_t)y * W + xb;
            if (xb + 3 < W && ((uintptr_t)o & 3) == 0) {
                *(unsigned int*)o = v;
            } else {
                for (int j = 0; j < 4; ++j)
                    if (xb + j < W) o[j] = (unsigned char)(v >> (8 * j));
            }
        }
    }
    if (tile_changed && lane == 0) atomicOr(flag, 1);
}

// ---- finish -------------------------------------------------------------------------------------------------------------------
template <int OC>
__global__ __launch_bounds__(NT) void canny_finish_kernel(const unsigned char* __restrict__ map, size_t total, unsigned char* __restrict__ out) {
    const size_t i4 = ((size_t)blockIdx.x * NT + threadIdx.x) * 4;
    if (i4 >= total) return;
    const unsigned char* p = map + i4;
    unsigned char* o = out + i4 * OC;
    if (i4 + 4 <= total && ((uintptr_t)p & 3) == 0 && ((uintptr_t)o & 3) == 0) {
        const unsigned int v = *(const unsigned int*)p;
        // a byte is 0, 1 or 2: bit 1 set <=> strong; spread it over the byte
        const unsigned int e = ((v >> 1) & 0x01010101u) * 255u;
        if (OC == 1) {
            *(unsigned int*)o = e;
        } else {
            const unsigned int e0 = e & 255u, e1 = (e >> 8) & 255u, e2 = (e >> 16) & 255u, e3 = e >> 24;
            ((unsigned int*)o)[0] = e0 * 0x00010101u | e1 << 24;
            ((unsigned int*)o)[1] = e1 * 0x00000101u | e2 * 0x01010000u;
            ((unsigned int*)o)[2] = e2 | e3 * 0x01010100u;
        }
    } else {
        for (int j = 0; j < 4 && i4 + j < total; ++j) {
            const unsigned char e = p[j] == 2 ? 255 : 0;
#pragma unroll
            for (int ch = 0; ch < OC; ++ch) o[j * OC + ch] = e;
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
int check_dims(const char* what, int N, int H, int W, int chans) {
    CTRL_CHECK(N >= 1 && H >= 1 && W >= 1, std::string(what) + ": N, H and W must be at least 1");
    // byte offsets are 64-bit, but pixel counts and the 1-D grids are int: one call handles up to 2^31 - 1 bytes of its largest tensor
    CTRL_CHECK((double)N * H * W * chans <= 2147483647.0, std::string(what) + ": N*H*W*channels exceeds 2^31 - 1 bytes; split the batch");
    const long tiles = (long)N * ((H + TH - 1) / TH) * ((W + TW - 1) / TW);
    CTRL_CHECK(tiles <= 2147483647L, std::string(what) + ": too many tiles for one launch; split the batch");
    return 0;
}
inline int tiles_of(int v, int tile) { return (v + tile - 1) / tile; }

int refuse_capture(const char* what, hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(s, &cs));
    CTRL_CHECK(cs == hipStreamCaptureStatusNone, std::string(what) + ": the stream is capturing; the hysteresis pass loop reads a flag back "
               "between launches and cannot be recorded into a graph");
    return 0;
}

std::mutex g_pin_mu;
int* g_pin[kMaxDevices] = {};        // pinned readback words, one block per device, allocated once

}  // namespace

void canny_launch_shape(int* tile_h, int* tile_w) { *tile_h = TH; *tile_w = TW; }

long canny_ws_bytes(int N, int H, int W) { return kFlagBytes + (((long)N * H * W + 255) / 256) * 256; }

int op_canny_map(const unsigned char* src, int N, int H, int W, int C, double low, double high, unsigned char* map, hipStream_t s) {
    CTRL_CHECK(src && map, "canny_map: null pointer");
    CTRL_CHECK(C == 1 || C == 3, "canny_map: C must be 1 or 3");
    TRY(check_dims("canny_map", N, H, W, C));
    CTRL_CHECK(!std::isnan(low) && !std::isnan(high), "canny_map: a threshold is NaN");
    if (low > high) { const double x = low; low = high; high = x; }        // cv::Canny: swap, then cvFloor
    // a magnitude lies in [0, 2040]: thresholds beyond [-1, 2041] compare like those two
    const int lo = (int)std::floor(std::fmin(std::fmax(low, -1.0), 2041.0)), hi = (int)std::floor(std::fmin(std::fmax(high, -1.0), 2041.0));
    const int tx = tiles_of(W, TW), ty = tiles_of(H, TH);
    const size_t total = (size_t)N * H * W * C;
    PROF_WORK(0, (double)total + (double)N * H * W);
    if (C == 3)
        LAUNCH("canny", canny_map_kernel<3>, dim3((unsigned)(N * ty * tx)), dim3(NT), 0, s, src, total, H, W, tx, ty, lo, hi, map);
    else
        LAUNCH("canny", canny_map_kernel<1>, dim3((unsigned)(N * ty * tx)), dim3(NT), 0, s, src, total, H, W, tx, ty, lo, hi, map);
    return 0;
}

int op_canny_hysteresis(unsigned char* map, int N, int H, int W, void* ws, long ws_bytes, int* passes, int* readbacks, hipStream_t s) {
    CTRL_CHECK(map && ws && passes && readbacks, "canny_hysteresis: null pointer");
    TRY(check_dims("canny_hysteresis", N, H, W, 1));
    CTRL_CHECK(ws_bytes >= kFlagBytes, "canny_hysteresis: the workspace is smaller than its flag block (256 bytes)");
    CTRL_CHECK(((uintptr_t)ws & 3) == 0, "canny_hysteresis: the workspace must be 4-byte aligned");
    *passes = 0; *readbacks = 0;
    TRY(refuse_capture("canny_hysteresis", s));
    std::lock_guard<std::mutex> lk(g_pin_mu);          // one readback block per device: calls on one device take turns
    const int dev = cur_device();
    if (!g_pin[dev]) HIP_TRY(hipHostMalloc((void**)&g_pin[dev], kFlagBytes, hipHostMallocDefault));
    volatile int* pin = g_pin[dev];
    int* flags = (int*)ws;
    const int batch = std::min(std::max(policy_int(P_CANNY_BATCH, 4), 1), kMaxBatch);
    const int tx = tiles_of(W, TW), ty = tiles_of(H, TH);
    // every pass but the last promotes a pixel in every image that has not settled, so H*W + 1 passes settle any batch
    const long cap = (long)H * W + 1;
    long done = 0;
    for (int rb = 1;; ++rb) {
        CTRL_CHECK(done < cap, "canny_hysteresis: no fixpoint after H*W + 1 passes (cannot happen: every pass is monotone)");
        HIP_TRY(hipMemsetAsync(flags, 0, kFlagBytes, s));
        for (int i = 0; i < batch; ++i) {
            PROF_WORK(0, 2.0 * N * H * W);
            LAUNCH("canny", canny_hyst_kernel, dim3((unsigned)(N * ty * tx)), dim3(64), 0, s, map, H, W, tx, ty, flags + i);
        }
        HIP_TRY(hipMemcpyAsync((void*)pin, flags, sizeof(int) * batch, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        *readbacks = rb;
        for (int i = 0; i < batch; ++i)
            if (pin[i] == 0) {                         // pass done + i + 1 promoted nothing: the passes behind it in this batch were idle
                *passes = (int)std::min(done + i + 1, 2147483647L);
                return 0;
            }
        done += batch;
    }
}

int op_canny_finish(const unsigned char* map, int N, int H, int W, int out_channels, unsigned char* out, hipStream_t s) {
    CTRL_CHECK(map && out, "canny_finish: null pointer");
    CTRL_CHECK(out_channels == 1 || out_channels == 3, "canny_finish: out_channels must be 1 or 3");
    TRY(check_dims("canny_finish", N, H, W, out_channels));
    const size_t total = (size_t)N * H * W;
    const unsigned blocks = (unsigned)((total + 4 * NT - 1) / (4 * NT));
    PROF_WORK(0, (double)total * (1 + out_channels));
    if (out_channels == 3) LAUNCH("canny", canny_finish_kernel<3>, dim3(blocks), dim3(NT), 0, s, map, total, out);
    else LAUNCH("canny", canny_finish_kernel<1>, dim3(blocks), dim3(NT), 0, s, map, total, out);
    return 0;
}

int op_canny(const unsigned char* src, int N, int H, int W, int C, double low, double high, int out_channels, unsigned char* out,
             void* ws, long ws_bytes, int* passes, int* readbacks, hipStream_t s) {
    CTRL_CHECK(src && out && ws && passes && readbacks, "canny: null pointer");
    CTRL_CHECK(C == 1 || C == 3, "canny: C must be 1 or 3");
    CTRL_CHECK(out_channels == 1 || out_channels == 3, "canny: out_channels must be 1 or 3");
    TRY(check_dims("canny", N, H, W, 3));
    CTRL_CHECK(ws_bytes >= canny_ws_bytes(N, H, W), "canny: the workspace is smaller than ctrl_canny_ws_bytes(N, H, W)");
    *passes = 0; *readbacks = 0;
    TRY(refuse_capture("canny", s));                   // before anything is enqueued
    unsigned char* map = (unsigned char*)ws + kFlagBytes;
    TRY(op_canny_map(src, N, H, W, C, low, high, map, s));
    TRY(op_canny_hysteresis(map, N, H, W, ws, kFlagBytes, passes, readbacks, s));
    return op_canny_finish(map, N, H, W, out_channels, out, s);
}
