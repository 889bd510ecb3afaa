// lws_systolic_layout.h -- the time-skewed HBM layout of the systolic engine and the passes that convert to and from it.
// The same for every build of the update kernel (lws_systolic.hip): a build enters through its row length and its skew only
// (run-time values: six pairs among the seventeen builds), so all of this is compiled once, in lws_systolic_driver.hip.
//
// The layout:  state_w[(SKEW m + c) mod G][m mod ROWL]  holds bin c < C = F - 1 of (extended) frame m -- a value is filed under
// the step at which the kernel's lane produces it, so that every access of a wave there is ROWL consecutive elements; amp_w
// holds the target magnitudes the same way, and the Nyquist bins (bin C does not fit the frame period) sit in state_nyq /
// amp_nyq[m].  Extended frames: the plan's Q - 1 edge-pad frames on either side of the T real ones.
//
// Both directions move 64 x 64 tiles (64 frames of one group x 64 production times) through LDS: in the caller's layouts a
// frame's bins are contiguous, in the skewed layout the lanes of a time step are, so the tile is read along one and written
// along the other and both sides of the copy are full 512-byte segments.  grid: (Kt * NT, B), see lws_systolic_geom.h; 256
// threads.  With ROWL = 128 (256) two (four) groups of 64 frames share the rows of the layout, with ROWL < 64 a group spans
// several rounds.
//
// fp16 storage (H16): the values are stored multiplied by store_scale(largest magnitude), so that magnitude has to be
// known before the first store -- a reduction pass of its own (k_amax) instead of the atomic maximum the fp32 kernels
// take on the way.  On the way out the state only contributes its PHASE: a bin that some sweep could have updated is
// returned with the fp32 target magnitude it was given (the caller's |S|), a bin no sweep could touch keeps the caller's
// value bit for bit; so fp16 storage costs phase accuracy, never magnitude accuracy.
#pragma once
#include "lws_systolic_store.h"

namespace lws {
namespace {

constexpr int TILE = SYS_TILE, TPAD = TILE + 1;

// The skewed layout of one call, as the layout passes see it.
struct Skew {
    int T, Q, C;                        // real frames; frames per stencil row; bins below the Nyquist bin
    int G, TpPad, NT, rowl_shift, skew;
    __device__ int Tp() const { return T + 2 * (Q - 1); }
    __device__ bool real_frame(int me) const { return me >= Q - 1 && me < T + Q - 1; }
    // the real frame an extended frame shows: the edge-pad frames repeat the first / last one
    __device__ int pad_source(int me) const {
        const int src = me - (Q - 1);
        return src < 0 ? 0 : (src > T - 1 ? T - 1 : src);
    }
    // where the value produced at (unwrapped) time tau of frame me lies in state_w / amp_w of its spectrogram
    __device__ size_t at(int tau, int me) const { return ((size_t)(tau % G) << rowl_shift) + (me & ((1 << rowl_shift) - 1)); }
};

// The tile of a block, and the cell of it a thread holds on either side of the transpose through ts[frame][time].
struct Tile {
    int kk, tt, b, tau0, wave, lane;    // group of 64 frames, time tile, spectrogram; first production time (before the mod G)
    __device__ explicit Tile(const Skew &s)
        : kk(blockIdx.x / s.NT), tt(blockIdx.x - kk * s.NT), b(blockIdx.y), tau0(s.skew * SYS_LANES * kk + TILE * tt),
          wave(threadIdx.x >> 6), lane(threadIdx.x & 63) {}
    __device__ bool has_nyquist() const { return tt == 0 && wave == 0; }   // ... lane l: the Nyquist bin of frame 64 kk + l
    __device__ int frame(int ml) const { return SYS_LANES * kk + ml; }
};
struct Cell {
    int me, c, tau;                     // frame, bin, production time
    bool in;                            // a bin of the layout (the tiles overhang it in frames and in time)
    __device__ Cell(const Skew &s, const Tile &t, int ml, int tl) : me(t.frame(ml)), c(t.tau0 + tl - s.skew * me), tau(t.tau0 + tl), in(me < s.Tp() && c >= 0 && c < s.C) {}
};
// frame side: wave w holds frames w, w + 4, ... of the tile, a lane one time of each (in the caller's layout: consecutive bins)
__device__ __forceinline__ Cell frame_side(const Skew &s, const Tile &t, int i) { return Cell(s, t, t.wave + 4 * i, t.lane); }
// time side: wave w holds times w, w + 4, ..., a lane one frame of each (in the skewed layout: consecutive elements)
__device__ __forceinline__ Cell time_side(const Skew &s, const Tile &t, int i) { return Cell(s, t, t.lane, t.wave + 4 * i); }

// spectrogram b's part of state_w / amp_w and of the Nyquist buffers (E: Store<H16>::cplx / real)
template <typename E> __device__ __forceinline__ E *skew_rows(const Skew &s, int b, void *base) { return static_cast<E *>(base) + ((size_t)b * s.G << s.rowl_shift); }
template <typename E> __device__ __forceinline__ E *nyq_row(const Skew &s, int b, void *base) { return static_cast<E *>(base) + (size_t)b * s.TpPad; }
// store a value and its target magnitude (sc: store_scale of the spectrogram; 1 for fp32 storage)
template <bool H16> __device__ __forceinline__ void store_cell(typename Store<H16>::cplx *s, typename Store<H16>::real *a, size_t idx, float2 v, float av, float sc) {
    if constexpr (H16) { s[idx] = pack_h2(make_float2(v.x * sc, v.y * sc)); a[idx] = pack_h(av * sc); }
    else { s[idx] = v; a[idx] = av; }
}
template <bool H16> __device__ __forceinline__ float2 load_cell(const typename Store<H16>::cplx *s, size_t idx) {
    if constexpr (H16) return unpack_h2(s[idx]);
    else return s[idx];
}

// |S| of a complex64 input exactly as k_prep forms it (fp64 square root, rounded once)
__device__ __forceinline__ float mag_of(float2 v, double *mag64 = nullptr) {
    const double m = sqrt((double)v.x * (double)v.x + (double)v.y * (double)v.y);
    if (mag64) *mag64 = m;
    return (float)m;
}
// fp16 storage, on the way out: the phase of the stored value v with the fp32 target magnitude a -- where there is a phase and
// some sweep of the call could have updated the bin (the kernel's own test, on the stored half value in the scaled domain:
// magnitude above the smallest threshold in effect, k_thr_min).  False: the bin keeps the caller's value.
__device__ __forceinline__ bool restore_h16(float2 v, float a, float sc, float thr_min, float2 *out) {
    const float m2 = v.x * v.x + v.y * v.y;
    const float s = a / sqrtf(m2);
    *out = make_float2(v.x * s, v.y * s);
    return m2 > 0.f && unpack_h(pack_h(a * sc)) > thr_min * sc;
}

// 256 threads: op over the block's values in a fixed tree (deterministic); the result in thread 0
template <typename T, typename Op> __device__ __forceinline__ T block_tree(T v, T *red, Op op) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s2 = 128; s2 > 0; s2 >>= 1) {
        if (threadIdx.x < s2) red[threadIdx.x] = op(red[threadIdx.x], red[threadIdx.x + s2]);
        __syncthreads();
    }
    return red[0];
}
// block max -> atomic max on the bit pattern (non-negative floats order like unsigned ints)
__device__ __forceinline__ void fold_block_max(unsigned *amax_bits, float mx, float *red) {
    const float m = block_tree(mx, red, [](float x, float y) { return fmaxf(x, y); });
    if (threadIdx.x == 0 && m > 0.f) atomicMax(amax_bits, __float_as_uint(m));
}
__device__ __forceinline__ double block_sum(double v, double *red) {
    return block_tree(v, red, [](double x, double y) { return x + y; });
}

// ---- the two ends a conversion can have on the caller's side ----------------------------------------------------------
// The extended buffers of the reference layout, [B][Tp][F + 2 L] with the magnitudes beside them (lws_generic.hip: k_prep).
struct Extended {
    static constexpr bool SUMS = false;
    float2 *state;
    const float *amp;
    int Np, L;
    __device__ size_t index(const Skew &s, int b, int me, int c) const { return ((size_t)b * s.Tp() + me) * Np + L + c; }
    __device__ bool holds(const Skew &s, int me) const { return me < s.Tp(); }
    __device__ float2 fetch(const Skew &s, int b, int me, int c, float *a) const { *a = amp[index(s, b, me, c)]; return state[index(s, b, me, c)]; }
    __device__ float magnitude(float2, float a, double *) const { return a; }
    __device__ float target(const Skew &s, int b, int me, int c, float2 *) const { return amp[index(s, b, me, c)]; }
    // also restores the Hermitian pad columns
    __device__ void put(const Skew &s, int b, int me, int c, float2 v) const {
        float2 *orow = state + index(s, b, me, -L);
        orow[L + c] = v;
        const float2 vc = make_float2(v.x, -v.y);
        if (c >= 1 && c <= L) orow[L - c] = vc;                        // image below DC
        if (c >= s.C - L && c < s.C) orow[L + 2 * s.C - c] = vc;       // image above Nyquist
    }
    __device__ void keep(const Skew &, int, int, int, float2) const {}   // in place: untouched bins stay as they are
};
// The caller's unpadded [B][T][F] complex64 spectrograms, for calls that are one batch stage: what k_prep + the extended
// conversion and that + k_extract do in two passes each.  Forms |S| on the way in; real frames only on
// the way out.  `in` may be the same buffer as `out`: every element is read and written by the same thread.
struct Callers {
    static constexpr bool SUMS = true;   // ... and sums |S| over the real frames in fp64, one partial sum per tile, for mean|S|
    const float2 *in;
    float2 *out;
    int F;
    __device__ size_t index(const Skew &s, int b, int me, int c) const { return ((size_t)b * s.T + s.pad_source(me)) * F + c; }
    __device__ bool holds(const Skew &s, int me) const { return s.real_frame(me); }
    __device__ float2 fetch(const Skew &s, int b, int me, int c, float *) const { return in[index(s, b, me, c)]; }
    __device__ float magnitude(float2 v, float, double *mag64) const { return mag_of(v, mag64); }
    __device__ float target(const Skew &s, int b, int me, int c, float2 *orig) const { *orig = in[index(s, b, me, c)]; return mag_of(*orig); }
    __device__ void put(const Skew &s, int b, int me, int c, float2 v) const { out[index(s, b, me, c)] = v; }
    __device__ void keep(const Skew &s, int b, int me, int c, float2 orig) const { out[index(s, b, me, c)] = orig; }
};

// largest magnitude of each spectrogram's n_per elements from p + b * stride (H16 only); grid (blocks, B)
__device__ __forceinline__ float amax_of(float a) { return a; }
__device__ __forceinline__ float amax_of(float2 v) { return mag_of(v); }
template <typename E> __global__ void __launch_bounds__(256) k_amax(const E *p, size_t stride, size_t n_per, unsigned *amax_bits) {
    __shared__ float red[256];
    p += (size_t)blockIdx.y * stride;
    float mx = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_per; i += (size_t)gridDim.x * 256) mx = fmaxf(mx, amax_of(p[i]));
    fold_block_max(amax_bits + blockIdx.y, mx, red);
}
// smallest threshold of each spectrogram that any of its bins exceeds (+inf if none): a bin whose stored magnitude is not
// above it is never updated by this call
__global__ void __launch_bounds__(64) k_thr_min(const float *thr, const float *amax, int n_iters, float *thr_min) {
    const int b = blockIdx.x;
    float m = __builtin_inff();
    for (int i = threadIdx.x; i < n_iters; i += 64) {
        const float th = thr[(size_t)b * n_iters + i];
        if (amax[b] > th) m = fminf(m, th);
    }
    for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o));
    if (threadIdx.x == 0) thr_min[b] = m;
}
// mean|S| of each spectrogram from the partial sums, fixed order
__global__ void __launch_bounds__(256) k_mean_partials(const double *partial, double *mean_amp, int n, double denom) {
    __shared__ double red[256];
    const int b = blockIdx.x;
    double acc = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) acc += partial[(size_t)b * n + i];
    const double sum = block_sum(acc, red);
    if (threadIdx.x == 0) mean_amp[b] = sum / denom;
}

// caller's layout -> skewed layout, with the largest target magnitude of the real frames (fp32 storage: folded into amax_bits
// here; H16: k_amax ran before).  gate: non-null -- run only if *gate != 0.
template <bool H16, typename Source>
__global__ void __launch_bounds__(256) k_to_skew(Source src, void *state_w, void *amp_w, void *state_nyq, void *amp_nyq,
                                                  unsigned *amax_bits, double *partial, Skew s, const int *gate) {
    __shared__ float2 ts[TILE][TPAD];
    __shared__ float ta[TILE][TPAD];
    __shared__ float red[256];
    if (gate != nullptr && *gate == 0) return;
    const Tile t(s);
    using ST = Store<H16>;
    typename ST::cplx *sw = skew_rows<typename ST::cplx>(s, t.b, state_w), *snq = nyq_row<typename ST::cplx>(s, t.b, state_nyq);
    typename ST::real *aw = skew_rows<typename ST::real>(s, t.b, amp_w), *anq = nyq_row<typename ST::real>(s, t.b, amp_nyq);
    const float sc = H16 ? store_scale(__uint_as_float(amax_bits[t.b])) : 1.f;
    float mx = 0.f;
    double msum = 0.0;                                       // this thread's share of sum |S| over the real frames
    // all of a thread's loads are issued before the first one is used: 16 x 512 bytes in flight per wave
    float2 vin[TILE / 4];
    float ain[TILE / 4];
#pragma unroll
    for (int i = 0; i < TILE / 4; ++i) {
        const Cell x = frame_side(s, t, i);
        ain[i] = 0.f;
        vin[i] = x.in ? src.fetch(s, t.b, x.me, x.c, &ain[i]) : make_float2(0.f, 0.f);
    }
    auto take = [&](int me, float2 v, float a) {             // a bin's magnitude, counted if its frame is a real one
        double mag = 0.0;
        const float av = src.magnitude(v, a, &mag);
        if (s.real_frame(me)) { mx = fmaxf(mx, av); msum += mag; }
        return av;
    };
#pragma unroll
    for (int i = 0; i < TILE / 4; ++i) {
        const Cell x = frame_side(s, t, i);
        ts[t.wave + 4 * i][t.lane] = vin[i];
        ta[t.wave + 4 * i][t.lane] = x.in ? take(x.me, vin[i], ain[i]) : 0.f;
    }
    if (t.has_nyquist()) {
        const int me = t.frame(t.lane);
        if (me < s.Tp()) {
            float a = 0.f;
            const float2 v = src.fetch(s, t.b, me, s.C, &a);
            store_cell<H16>(snq, anq, me, v, take(me, v, a), sc);
        }
    }
    __syncthreads();
    for (int i = 0; i < TILE / 4; ++i) {
        const Cell x = time_side(s, t, i);
        if (x.in) store_cell<H16>(sw, aw, s.at(x.tau, x.me), ts[t.lane][t.wave + 4 * i], ta[t.lane][t.wave + 4 * i], sc);
    }
    if constexpr (!H16) fold_block_max(amax_bits + t.b, mx, red);
    if constexpr (Source::SUMS) {
        __shared__ double dred[256];
        const double sum = block_sum(msum, dred);
        if (threadIdx.x == 0) partial[(size_t)t.b * gridDim.x + blockIdx.x] = sum;   // one partial sum per tile
    }
}

// skewed layout -> caller's layout.  fp32 storage: every bin the sink holds; H16: see restore_h16.
template <bool H16, typename Sink>
__global__ void __launch_bounds__(256) k_from_skew(Sink dst, void *state_w, void *state_nyq, const float *amax,
                                                    const float *thr_min, Skew s) {
    __shared__ float2 ts[TILE][TPAD];
    const Tile t(s);
    using ST = Store<H16>;
    const typename ST::cplx *sw = skew_rows<typename ST::cplx>(s, t.b, state_w), *snq = nyq_row<typename ST::cplx>(s, t.b, state_nyq);
    const float sc = H16 ? store_scale(amax[t.b]) : 1.f, tmin = H16 ? thr_min[t.b] : 0.f;
    float2 vin[TILE / 4];
#pragma unroll
    for (int i = 0; i < TILE / 4; ++i) {           // all loads first
        const Cell x = time_side(s, t, i);
        vin[i] = x.in ? load_cell<H16>(sw, s.at(x.tau, x.me)) : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < TILE / 4; ++i) ts[t.lane][t.wave + 4 * i] = vin[i];
    __syncthreads();
    auto give = [&](int me, int c, float2 v) {
        if constexpr (H16) {     // phase from the fp16 state, magnitude from the fp32 target
            float2 orig = make_float2(0.f, 0.f), r;
            const float a = dst.target(s, t.b, me, c, &orig);
            if (restore_h16(v, a, sc, tmin, &r) && s.real_frame(me)) dst.put(s, t.b, me, c, r);
            else dst.keep(s, t.b, me, c, orig);
        } else {
            dst.put(s, t.b, me, c, v);
        }
    };
    for (int i = 0; i < TILE / 4; ++i) {
        const Cell x = frame_side(s, t, i);
        if (x.in && dst.holds(s, x.me)) give(x.me, x.c, ts[t.wave + 4 * i][t.lane]);
    }
    if (t.has_nyquist()) {
        const int me = t.frame(t.lane);
        if (dst.holds(s, me)) give(me, s.C, load_cell<H16>(snq, me));
    }
}

}  // namespace
}  // namespace lws
