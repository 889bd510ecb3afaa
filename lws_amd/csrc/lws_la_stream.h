// lws_la_stream.h -- the step clock of a look-ahead stream (lws_rtisi_stream and lws_misi_stream of lws_gla.hip): everything such a
// stream decides on the host that is arithmetic rather than HIP.  Plain C++ with no HIP include, so that the CPU tests compile the
// same text with g++ (tests/test_la_stream_clock.py).  Internal linkage, as lws_fft.h, which includes this.
//
// A stream takes frames in pushes of any size and commits frame m once frame m + LA has entered; finish() commits the rest.  The
// clock holds the counts between the calls.  la_plan_push / la_plan_finish say what a call does -- whether it launches, every kernel
// argument, which held buffers are read and written, what the caller gets back, the clock after it -- and change nothing: the handle
// launches, checks the launch, and only then takes `after`.  A call that is refused or fails leaves the stream as it was.
#pragma once

#include <cstddef>

namespace {

// N = odd * 2^log2e
struct Factors { int odd, log2e; };
Factors factor(int n) { Factors f{n, 0}; while (!(f.odd & 1)) { f.odd >>= 1; ++f.log2e; } return f; }
int prepad(int N, int hop) { const int r = N % hop; return r == 0 ? N - hop : N - r; }   // lws.pyx:55-60

// The arguments of k_rtisi_stream and k_misi_la_stream (their comments in lws_la_stream_kernels.h say what the kernels do with them).
struct RtisiStreamArgs {
    int N, odd, log2e, hop, LA, iters;
    int nsteps, Mrel;            // steps of this launch; frames from its first step to the end of the stream (nsteps + LA while open)
    int closing, origin;         // the launch that ends the stream; the first step is frame 0 of the stream
    int zero_lo, emit_end;       // the lead-in cut and the end of the emitted samples, from the first sample of the first step
    int base, slot_m, cur;       // ring offset and slot of the first step's frame; which frame buffer is fcur (scratch placement)
    int nheld, held_rows;        // held frames in front of the chunk's; row stride of a stream in the held buffers
    int chunk_rows, out_rows, out_samples;   // rows per stream of S / A, of Cout, samples per stream of xout
    size_t state_floats;         // stride of a stream in `state`
};
struct MisiStreamArgs {
    RtisiStreamArgs r;   // r.state_floats: stride of ONE source in `state`; the rows are [B][K][rows][F], the samples [B][K][samples]
    int K, frame0;       // sources; the stream's first frame, counted from the first step's (clamped: no earlier frame covers sample 0)
    int ny_held, ny_chunk, y_rows, y_keep;   // mixture samples held / in the chunk, per-stream stride of held.y, samples to keep
    size_t stream_floats;                    // stride of a stream in `state`
};

// floats of one spectrogram's state with both frame buffers: the ring of R = N + LA hop, and 2 (LA + 1) frames
size_t la_state_floats(int N, int hop, int LA) { return (size_t)N + (size_t)LA * hop + 2 * (size_t)(LA + 1) * N; }

struct LaClock {
    // what create fixes.  K == 0: no mixture (RTISI-LA).  lo: the lead-in perfectrec cuts.  given: the start rows are read
    int N = 0, hop = 0, LA = 0, iters = 0, K = 0, lo = 0, perfectrec = 0, given = 1;
    size_t state_floats = 0, stream_floats = 0;   // strides in `state` of one spectrogram and (K > 0) of one mixture: the placement's
    int y_rows = 0;                               // floats of a stream in held_y
    // what the calls move
    long long entered = 0, committed = 0;   // frames pushed, frames committed
    int base = 0, slot = 0, cur = 0;        // of the next step: ring offset, slot of its frame, which frame buffer is fcur
    int held = 0;                           // which held buffers are current
    bool ran = false, finished = false;
};

enum LaRefusal { LA_GO = 0, LA_NEGATIVE, LA_FINISHED, LA_TOO_LONG, LA_SAMPLES };

// the look-ahead create refuses: the kernels count samples of a launch, and (K > 0) floats of a mixture's state, in ints
bool la_look_ahead_fits(int N, int hop, int LA, int K) {
    if ((long long)(LA + 2) * hop + N > 0x7fffffffLL / 2) return false;
    return K == 0 || 2 * ((size_t)K + 1) * la_state_floats(N, hop, LA) <= 0x7fffffffULL;
}

void la_clock_init(LaClock &c, int N, int hop, int LA, int iters, int K, bool perfectrec, bool given, bool in_lds) {
    c = LaClock{};
    c.N = N; c.hop = hop; c.LA = LA; c.iters = iters; c.K = K; c.perfectrec = perfectrec ? 1 : 0; c.given = given ? 1 : 0;
    c.lo = perfectrec ? prepad(N, hop) : 0;
    // IN_LDS keeps the other frame buffer, and target and xs of a mixture, in LDS alone
    const size_t R = (size_t)N + (size_t)LA * hop;
    c.state_floats = la_state_floats(N, hop, LA) - (in_lds ? (size_t)(LA + 1) * N : 0);
    c.stream_floats = (size_t)K * c.state_floats + (in_lds ? 0 : ((size_t)K + 1) * R);
    // held samples: the R - hop the next launch still needs; before the first launch, the lead-in (never read) and what was stashed
    const size_t keep = R - hop;
    c.y_rows = K ? (int)(keep > (size_t)c.lo ? keep : (size_t)c.lo) + 1 : 0;
}

// mixture samples under the first M frames of a stream
long long la_need(const LaClock &c, long long M) { return M <= 0 || c.K == 0 ? 0 : (long long)c.hop * (M - 1) + c.N - c.lo; }

// the steps a push of `frames` commits
long long la_push_steps(const LaClock &c, int frames) {
    const long long entered = c.entered + frames;
    return entered > c.LA ? entered - c.LA - c.committed : 0;
}

// whether a push may go ahead; *want: the mixture samples it must carry
LaRefusal la_check_push(const LaClock &c, int frames, int samples, long long *want) {
    *want = 0;
    if (frames < 0) return LA_NEGATIVE;
    if (c.finished) return LA_FINISHED;
    if (((long long)frames + c.LA + 2) * c.hop + c.N > 0x7fffffffLL) return LA_TOO_LONG;
    *want = la_need(c, c.entered + frames) - la_need(c, c.entered);
    return c.K && samples != *want ? LA_SAMPLES : LA_GO;
}

struct LaPlan {
    bool launch;                   // false: a push only stashes its rows and samples, a finish has nothing left to run
    int stash_row, stash_y;        // (push, no launch) where the chunk goes in the held buffers `write`: row, mixture sample
    MisiStreamArgs a;              // (launch) a.r alone for K == 0
    int read, write;               // the held buffers a launch reads, and the ones the call writes
    bool keep_s, keep_a, keep_y;   // (launch) which of S_next / A_next / y_next the kernel gets
    int frames_out, samples_out;   // what the call reports
    LaClock after;
};

// the commit steps committed .. committed + nsteps - 1; M < 0 while the stream is open, the frame count at its end
void la_plan_launch(const LaClock &c, LaPlan &p, int frames, int samples, int out_rows, int out_samples, int nsteps, long long M) {
    const bool closing = M >= 0;
    const int LA = (closing && !c.ran) ? (int)M - 1 : c.LA;   // an end before the first commit: no frame beyond M - 1 to look at
    const Factors fc = factor(c.N);
    const long long t0 = (long long)c.hop * c.committed;
    const int R = c.N + LA * c.hop, back = c.N / c.hop + 1;
    p.launch = true;
    RtisiStreamArgs &q = p.a.r;
    q.N = c.N; q.odd = fc.odd; q.log2e = fc.log2e; q.hop = c.hop; q.LA = LA; q.iters = c.iters;
    q.nsteps = nsteps;
    q.Mrel = closing ? (int)(M - c.committed) : nsteps + LA;
    q.closing = closing;
    q.origin = c.committed == 0;
    q.zero_lo = c.lo > t0 ? (int)(c.lo - t0) : 0;
    q.emit_end = closing && c.perfectrec ? (int)((long long)c.hop * M - t0) : 0x7fffffff;
    q.base = c.base; q.slot_m = c.slot; q.cur = c.cur;
    q.nheld = c.ran ? c.LA : (int)c.entered;   // before the first launch: the stashed frames (the chunk's are not counted yet)
    q.held_rows = c.LA;
    q.chunk_rows = frames; q.out_rows = out_rows; q.out_samples = out_samples;
    q.state_floats = c.state_floats;
    p.a.K = c.K;
    p.a.frame0 = c.committed < back ? -(int)c.committed : -back;
    p.a.ny_held = c.ran ? R - c.hop : (int)(c.lo + la_need(c, c.entered));
    p.a.ny_chunk = samples;
    p.a.y_rows = c.y_rows;
    p.a.y_keep = R - c.hop;
    p.a.stream_floats = c.stream_floats;
    p.read = c.held; p.write = c.held ^ 1;
    p.keep_s = !closing && c.iters == 0;
    p.keep_a = !closing && !(c.given && c.iters == 0);   // any other start projects at entry: it keeps the magnitudes without iterations too
    p.keep_y = !closing && c.K > 0;
    const long long from = c.lo > t0 ? c.lo : t0;
    const long long to = !closing ? (long long)c.hop * (c.committed + nsteps) : c.perfectrec ? (long long)c.hop * M : (long long)c.hop * (M - 1) + c.N;
    p.frames_out = nsteps;
    p.samples_out = to > from ? (int)(to - from) : 0;
    p.after.base = (int)(((long long)c.base + (long long)c.hop * nsteps) % R);
    p.after.slot = (int)(((long long)c.slot + nsteps) % (LA + 1));
    p.after.cur = c.cur ^ (int)(((long long)c.iters * nsteps) & 1);
    p.after.held = p.write;
    p.after.committed = c.committed + nsteps;
    p.after.ran = true;
}

// a push of frames > 0 that la_check_push let through
LaPlan la_plan_push(const LaClock &c, int frames, int samples) {
    LaPlan p{};
    p.after = c;
    const long long nsteps = la_push_steps(c, frames);
    if (nsteps > 0) {
        la_plan_launch(c, p, frames, samples, frames, frames * c.hop, (int)nsteps, -1);
    } else {   // the frames that arrive before the first commit can run.  Held sample t is sample t of the stream's timeline
        p.write = c.held;
        p.stash_row = (int)c.entered;
        p.stash_y = (int)(c.lo + la_need(c, c.entered));
    }
    p.after.entered = c.entered + frames;
    return p;
}

LaRefusal la_check_finish(const LaClock &c) { return c.finished ? LA_FINISHED : LA_GO; }

// a finish that la_check_finish let through; want_signal: the caller takes the samples
LaPlan la_plan_finish(const LaClock &c, bool want_signal) {
    LaPlan p{};
    p.after = c;
    const long long M = c.entered, nsteps = M - c.committed;
    // no step left (nothing pushed, or look_ahead == 0): only the samples behind the last commit, which perfectrec cuts
    if (nsteps == 0 && (M == 0 || c.perfectrec || !want_signal))
        p.samples_out = M > 0 && !c.perfectrec ? c.N - c.hop : 0;
    else
        la_plan_launch(c, p, 0, 0, c.LA, c.N + c.LA * c.hop, (int)nsteps, M);
    p.after.finished = true;
    return p;
}

}  // namespace
