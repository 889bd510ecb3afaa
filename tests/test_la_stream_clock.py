"""CPU: the step clock of the look-ahead streams (lws_amd/csrc/lws_la_stream.h), the host arithmetic of lws_rtisi_stream and
lws_misi_stream.  The header is plain C++: compiled here with g++ behind a small shim, no GPU needed.

Whole streams are driven through the clock -- pushes in chunks, then finish -- and after every call what the clock planned is
compared with a restatement in Python.  The clock moves its state by incremental updates; the restatement is written as closed
forms in the absolute counts (c: frames committed before the call, e: frames entered before it), so the two cannot share a mistake."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "lws_amd", "csrc")
BUILD = os.path.join(HERE, "_build")

ARGS = ("N", "odd", "log2e", "hop", "LA", "iters", "nsteps", "Mrel", "closing", "origin", "zero_lo", "emit_end", "base", "slot_m", "cur",
        "nheld", "held_rows", "chunk_rows", "out_rows", "out_samples", "state_floats", "K", "frame0", "ny_held", "ny_chunk", "y_rows",
        "y_keep", "stream_floats")
PLAN = ("launch", "stash_row", "stash_y") + ARGS + ("read", "write", "keep_s", "keep_a", "keep_y", "frames_out", "samples_out")
STATE = ("entered", "committed", "base", "slot", "cur", "held", "ran", "finished")
GO, NEGATIVE, FINISHED, TOO_LONG, SAMPLES = range(5)

SHIM = r"""
#include "lws_la_stream.h"
static LaPlan last;
static void dump(const LaPlan &p, long long *o) {
    const RtisiStreamArgs &q = p.a.r;
    const long long v[] = {p.launch, p.stash_row, p.stash_y, q.N, q.odd, q.log2e, q.hop, q.LA, q.iters, q.nsteps, q.Mrel, q.closing, q.origin,
                           q.zero_lo, q.emit_end, q.base, q.slot_m, q.cur, q.nheld, q.held_rows, q.chunk_rows, q.out_rows, q.out_samples,
                           (long long)q.state_floats, p.a.K, p.a.frame0, p.a.ny_held, p.a.ny_chunk, p.a.y_rows, p.a.y_keep,
                           (long long)p.a.stream_floats, p.read, p.write, p.keep_s, p.keep_a, p.keep_y, p.frames_out, p.samples_out};
    for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) o[i] = v[i];
}
extern "C" {
LaClock *clock_new(int N, int hop, int LA, int iters, int K, int perfectrec, int given, int in_lds) {
    LaClock *c = new LaClock;
    la_clock_init(*c, N, hop, LA, iters, K, perfectrec != 0, given != 0, in_lds != 0);
    return c;
}
void clock_free(LaClock *c) { delete c; }
void clock_state(const LaClock *c, long long *o) {
    const long long v[] = {c->entered, c->committed, c->base, c->slot, c->cur, c->held, c->ran, c->finished};
    for (int i = 0; i < 8; ++i) o[i] = v[i];
}
long long clock_need(const LaClock *c, long long M) { return la_need(*c, M); }
long long clock_push_steps(const LaClock *c, int frames) { return la_push_steps(*c, frames); }
int look_ahead_fits(int N, int hop, int LA, int K) { return la_look_ahead_fits(N, hop, LA, K); }
// as the handle: the refusal if any, nothing planned for no frames, else the plan (kept for clock_commit)
int clock_plan_push(const LaClock *c, int frames, int samples, long long *want, long long *plan) {
    const LaRefusal r = la_check_push(*c, frames, samples, want);
    if (r != LA_GO || frames == 0) return r;
    last = la_plan_push(*c, frames, samples);
    dump(last, plan);
    return LA_GO;
}
int clock_plan_finish(const LaClock *c, int want_signal, long long *plan) {
    const LaRefusal r = la_check_finish(*c);
    if (r != LA_GO) return r;
    last = la_plan_finish(*c, want_signal != 0);
    dump(last, plan);
    return LA_GO;
}
void clock_commit(LaClock *c) { *c = last.after; }
}
"""


@pytest.fixture(scope="module")
def lib():
    os.makedirs(BUILD, exist_ok=True)
    so, shim = os.path.join(BUILD, "libla_stream_clock.so"), os.path.join(BUILD, "la_stream_clock_shim.cpp")
    with open(shim, "w") as f:
        f.write(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, shim, "-o", so], check=True)
    L = C.CDLL(so)
    ll, ip, vp = C.c_longlong, C.c_int, C.c_void_p
    L.clock_new.restype, L.clock_new.argtypes = vp, [ip] * 8
    L.clock_free.argtypes = [vp]
    L.clock_state.argtypes = [vp, C.POINTER(ll)]
    L.clock_need.restype, L.clock_need.argtypes = ll, [vp, ll]
    L.clock_push_steps.restype, L.clock_push_steps.argtypes = ll, [vp, ip]
    L.look_ahead_fits.argtypes = [ip] * 4
    L.clock_plan_push.argtypes = [vp, ip, ip, C.POINTER(ll), C.POINTER(ll)]
    L.clock_plan_finish.argtypes = [vp, ip, C.POINTER(ll)]
    L.clock_commit.argtypes = [vp]
    return L


class Clock(object):
    def __init__(self, lib, N, hop, LA, iters, K, perfectrec, given, in_lds):
        self.lib, self.h = lib, lib.clock_new(N, hop, LA, iters, K, int(perfectrec), int(given), int(in_lds))

    def state(self):
        v = (C.c_longlong * len(STATE))()
        self.lib.clock_state(self.h, v)
        return dict(zip(STATE, v))

    def plan_push(self, frames, samples):
        """(refusal, samples wanted, plan or None); the clock must not move."""
        before, want, v = self.state(), C.c_longlong(-1), (C.c_longlong * len(PLAN))()
        r = self.lib.clock_plan_push(self.h, frames, samples, C.byref(want), v)
        assert self.state() == before
        return r, want.value, dict(zip(PLAN, v)) if r == GO and frames else None

    def plan_finish(self, want_signal):
        before, v = self.state(), (C.c_longlong * len(PLAN))()
        r = self.lib.clock_plan_finish(self.h, int(want_signal), v)
        assert self.state() == before
        return r, dict(zip(PLAN, v)) if r == GO else None

    def commit(self):
        self.lib.clock_commit(self.h)

    def close(self):
        self.lib.clock_free(self.h)


def lead_in(N, hop, perfectrec):
    return (N - hop if N % hop == 0 else N - N % hop) if perfectrec else 0


def need(N, hop, perfectrec, K, M):
    return 0 if M <= 0 or K == 0 else hop * (M - 1) + N - lead_in(N, hop, perfectrec)


def istft_length(T, N, hop, perfectrec):
    """lws_istft_length: the overlap-added frames, less with perfectrec the lead-in and the last N - hop samples"""
    return hop * (T - 1) + N - (lead_in(N, hop, True) + N - hop if perfectrec else 0)


def expected(cfg, c, e, frames, samples, M):
    """The launch of a call with c frames committed and e entered before it: a push of `frames` (M None), or the finish at M frames."""
    N, hop, LA, iters, K, pr, given, in_lds = cfg
    lo, closing, ran = lead_in(N, hop, pr), M is not None, c > 0   # only the closing launch can run no step, and nothing follows it
    LA_eff = M - 1 if closing and not ran else LA
    R, R0 = N + LA_eff * hop, N + LA * hop
    nsteps = M - c if closing else max(0, e + frames - LA) - c
    odd = N
    while odd % 2 == 0:
        odd //= 2
    state = R0 + (LA + 1) * N * (1 if in_lds else 2)
    if closing:
        end = hop * M if pr else hop * (M - 1) + N
    else:
        end = hop * (c + nsteps)
    return dict(
        launch=1, N=N, odd=odd, log2e=(N // odd).bit_length() - 1, hop=hop, LA=LA_eff, iters=iters, nsteps=nsteps,
        Mrel=M - c if closing else nsteps + LA, closing=int(closing), origin=int(c == 0), base=hop * c % R, slot_m=c % (LA_eff + 1),
        cur=(iters * c) & 1, zero_lo=max(lo - hop * c, 0), emit_end=hop * M - hop * c if closing and pr else 0x7fffffff,
        nheld=LA if ran else e, held_rows=LA, chunk_rows=0 if closing else frames, out_rows=LA if closing else frames,
        out_samples=N + LA * hop if closing else frames * hop, state_floats=state, K=K, frame0=-min(c, N // hop + 1),
        ny_held=R - hop if ran else lo + need(N, hop, pr, K, e), ny_chunk=samples, y_rows=max(R0 - hop, lo) + 1 if K else 0, y_keep=R - hop,
        stream_floats=K * state + (0 if in_lds else (K + 1) * R0),
        keep_s=int(not closing and iters == 0), keep_a=int(not closing and not (given and iters == 0)), keep_y=int(not closing and K > 0),
        frames_out=nsteps, samples_out=max(0, end - max(hop * c, lo)), LA_eff=LA_eff)


def run_stream(lib, cfg, T, chunks, want_signal=True):
    """Drive one stream; returns {frame: (ring offset, slot, which buffer is fcur)} of its commits."""
    N, hop, LA, iters, K, pr, given, in_lds = cfg
    assert sum(chunks) == T
    clk = Clock(lib, *cfg)
    c = e = asked = got_frames = got_samples = 0
    written, launched, steps = 0, False, {}   # held buffers last written; the stashes go where a fresh clock reads

    def check_launch(p, want, c):
        want = dict(want)
        LA_eff = want.pop("LA_eff")
        for k, v in want.items():
            assert p[k] == v, (cfg, T, chunks, k, p[k], v)
        assert p["read"] == written and p["write"] == 1 - p["read"], (cfg, T, chunks, p["read"], p["write"], written)
        for i in range(p["nsteps"]):
            steps[c + i] = ((p["base"] + hop * i) % (N + LA_eff * hop), (p["slot_m"] + i) % (LA_eff + 1), p["cur"] ^ ((iters * i) & 1))

    for frames in chunks:
        ns = need(N, hop, pr, K, e + frames) - need(N, hop, pr, K, e)
        if K and ns > 0:   # a sample too few: refused, and (plan_push asserts it) the clock as it was
            assert clk.plan_push(frames, ns - 1)[0] == SAMPLES
        r, want, p = clk.plan_push(frames, ns)
        assert (r, want) == (GO, ns)
        assert lib.clock_push_steps(clk.h, frames) == max(0, e + frames - LA) - c
        asked += want
        if frames == 0:
            assert p is None
            continue
        nsteps = max(0, e + frames - LA) - c
        if nsteps > 0:
            check_launch(p, expected(cfg, c, e, frames, ns, None), c)
            written, launched = p["write"], True
        else:
            assert not launched   # once the look-ahead is full every push commits
            assert (p["launch"], p["stash_row"], p["stash_y"], p["write"]) == (0, e, lead_in(N, hop, pr) + need(N, hop, pr, K, e), written)
            assert (p["frames_out"], p["samples_out"]) == (0, 0)
        clk.commit()
        c, e = c + nsteps, e + frames
        got_frames, got_samples = got_frames + p["frames_out"], got_samples + p["samples_out"]
        st = clk.state()
        assert (st["entered"], st["committed"], st["ran"], st["finished"]) == (e, c, int(launched), 0)
    r, p = clk.plan_finish(want_signal)
    assert r == GO
    idle = e == c and (e == 0 or pr or not want_signal)   # no step left, and no sample behind the last commit to hand out
    assert p["launch"] == (0 if idle else 1), (cfg, T, chunks, want_signal)
    if idle:
        assert (p["frames_out"], p["samples_out"]) == (0, N - hop if e > 0 and not pr else 0)
    else:
        check_launch(p, expected(cfg, c, e, 0, 0, e), c)
    clk.commit()
    got_frames, got_samples = got_frames + p["frames_out"], got_samples + p["samples_out"]
    st = clk.state()
    assert (st["entered"], st["committed"], st["finished"]) == (T, c + p["frames_out"], 1)
    # after the end: everything is refused and nothing moves
    assert clk.plan_finish(want_signal)[0] == FINISHED
    assert clk.plan_push(1, need(N, hop, pr, K, T + 1) - need(N, hop, pr, K, T))[0] == FINISHED
    assert clk.plan_push(0, 0)[0] == FINISHED
    clk.close()
    assert got_frames == T
    assert got_samples == max(istft_length(T, N, hop, pr), 0)
    assert asked == need(N, hop, pr, K, T)
    assert sorted(steps) == list(range(T))
    return steps


def chunkings(T, rng):
    out = [[T], [1] * T]
    if T >= 3:
        out.append([2, 0, 1, T - 3])
    for _ in range(4):   # a handful of random cuts, empty pushes among them
        cuts = sorted(rng.integers(0, T + 1, size=int(rng.integers(1, 5))))
        out.append([int(b - a) for a, b in zip([0] + cuts, cuts + [T])])
    return out


@pytest.mark.parametrize("N,hop,perfectrec", [(64, 16, True), (48, 16, False), (256, 96, True), (64, 8, True), (64, 64, False)])
def test_streams_follow_the_closed_forms(lib, N, hop, perfectrec):
    rng = np.random.default_rng(N * 1000 + hop)
    for LA in (0, 1, 3, 5):
        for T in sorted({t for t in (1, 2, LA, LA + 1, LA + 2, 12) if t > 0}):
            cuts = chunkings(T, rng)
            for iters in (0, 2, 3):
                for K in (0, 3):
                    for given in (True, False):
                        cfg = (N, hop, LA, iters, K, perfectrec, given, (LA + K) % 2 == 0)   # either placement: only the strides differ
                        runs = [run_stream(lib, cfg, T, ch) for ch in cuts]
                        for ch, steps in zip(cuts, runs):   # where a frame's commit finds its state does not depend on the chunking
                            assert steps == runs[0], (cfg, T, ch)
                        run_stream(lib, cfg, T, cuts[-1], want_signal=False)


def test_refusals_leave_the_clock_alone(lib):
    clk = Clock(lib, 64, 16, 3, 2, 3, True, True, True)
    assert clk.plan_push(-1, 0)[0] == NEGATIVE
    assert clk.plan_push(2, 0)[0] == SAMPLES            # 2 frames carry hop + N - lead-in samples
    r, want, p = clk.plan_push(2, 16 + 64 - 48)
    assert (r, want, p["launch"]) == (GO, 32, 0)
    assert clk.plan_push((0x7fffffff - 64) // 16 - 4, 0)[0] == TOO_LONG   # (frames + LA + 2) hop + N beyond an int
    assert clk.plan_push((0x7fffffff - 64) // 16 - 5, 0)[0] == SAMPLES
    assert clk.state() == dict(zip(STATE, [0] * len(STATE)))   # none of this was committed
    clk.close()
    # create: (LA + 2) hop + N within half an int; with sources, twice (K + 1) states of R + 2 (LA + 1) N floats within an int
    half = 0x7fffffff // 2
    assert lib.look_ahead_fits(64, 16, (half - 64) // 16 - 2, 0) == 1 and lib.look_ahead_fits(64, 16, (half - 64) // 16 - 1, 0) == 0
    LA = next(la for la in range(1, 1 << 22) if 2 * 4 * (4096 + la * 1024 + 2 * (la + 1) * 4096) > 0x7fffffff)
    assert lib.look_ahead_fits(4096, 1024, LA - 1, 3) == 1 and lib.look_ahead_fits(4096, 1024, LA, 3) == 0
    assert lib.look_ahead_fits(4096, 1024, LA, 0) == 1
