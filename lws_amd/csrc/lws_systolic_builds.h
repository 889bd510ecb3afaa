// lws_systolic_builds.h -- the builds of lws_systolic.hip, one row each.  Preprocessor only: lws_systolic.hip takes its switches from
// the row that -DLWS_BUILD=<name> selects (none: narrow), lws_systolic.h declares one entry per row, lws_capi.hip walks them in order.
// A new build is one row, its name in LWS_SYSTOLIC_BUILDS below and in SYSTOLIC_BUILDS of the Makefile (object lws_systolic_<name>.o):
// the layout passes and the host driver (lws_systolic_driver.hip, compiled once) take its row length, skew, lag, slots and waves per slot
// as numbers, from its entry.
//
// The switches (what they mean: lws_systolic.hip) -- WIDE: 1 / 2 = two / four waves per sweep slot; Q8: 64-step ring, halo of 7, helper
// waves; SPW: sweep slots per wave; L7: frames 16 steps apart; R16: 16-step ring; TW: twiddles from a table; TWQ: ring of 8 TWQ steps.
// `slots` is the number of sweep slots the LDS holds (-DLWS_NSLOTS=n overrides it: experiments); `tag` goes into the kernel's name,
// systolic<tag>_q<Q>_l<L>_<kind>.
//
//                           namespace        tag          WIDE Q8 SPW L7 R16 TW TWQ slots
#define LWS_BUILD_quarter_q2 lws::quarter_q2, "_quarter_r16", 0, 0, 4, 0, 1, 0, 0, 44   // Q = 2 on the 16-step ring, frames of up to 129 bins (44 slots on 11 waves)
#define LWS_BUILD_quarter    lws::quarter,    "_quarter",     0, 0, 4, 0, 0, 0, 0, 24   // frames of up to 129 bins, four sweep slots per wave (25 ring sets of 6 KB are what the LDS holds)
#define LWS_BUILD_half_q2    lws::half_q2,    "_half_r16",    0, 0, 2, 0, 1, 0, 0, 26   // Q = 2 on the 16-step ring, frames of up to 257 bins (26 slots on 13 waves)
#define LWS_BUILD_half       lws::half,       "_half",        0, 0, 2, 0, 0, 0, 0, 14   // frames of up to 257 bins, two sweep slots per wave
#define LWS_BUILD_q2         lws::q2,         "_r16",         0, 0, 1, 0, 1, 0, 0, 15   // Q = 2 on a 16-step ring, frames of up to 513 bins
#define LWS_BUILD_narrow     lws,             "",             0, 0, 1, 0, 0, 0, 0, 7    // Q in {2, 4}, frames of up to 513 bins
#define LWS_BUILD_q8         lws::q8,         "",             0, 1, 1, 0, 0, 0, 0, 2    // Q = 8, 64-step ring, a main and two helper waves per slot
#define LWS_BUILD_wide_q2    lws::wide_q2,    "_wide_r16",    1, 0, 1, 0, 1, 0, 0, 7    // Q = 2 on the 16-step ring, frames of up to 1025 bins (two waves per slot)
#define LWS_BUILD_wide       lws::wide,       "_wide",        1, 0, 1, 0, 0, 0, 0, 3    // frames of up to 1025 bins, two waves per sweep slot
#define LWS_BUILD_xwide      lws::xwide,      "_xwide",       2, 0, 1, 0, 0, 0, 0, 1    // frames of up to 2049 bins, four waves per sweep slot
#define LWS_BUILD_l7         lws::l7,         "",             0, 0, 1, 1, 0, 0, 0, 3    // L = 6, 7 (frames 16 steps apart, 64-step ring), frames of up to 513 bins
// ... then the table-twiddle builds: Q = 3, and general weights of a hop that does not divide the frame (Q <= 4)
#define LWS_BUILD_tw_half    lws::tw_half,    "_half",        0, 0, 2, 0, 0, 1, 0, 14   // frames of up to 257 bins (25 ms / 10 ms speech framing)
#define LWS_BUILD_tw         lws::tw,         "",             0, 0, 1, 0, 0, 1, 0, 7    // frames of up to 513 bins
#define LWS_BUILD_tw_wide    lws::tw_wide,    "_wide",        1, 0, 1, 0, 0, 1, 0, 3    // frames of up to 1025 bins (two waves per sweep slot)
// ... and ceil(frame / hop) in 5..8 (exactly 5 / 6 frames per stencil row: the builds with their own ring depth first)
#define LWS_BUILD_tw_q5      lws::tw_q5,      "_r40",         0, 1, 1, 0, 0, 1, 5, 3    // 5 frames per row, 40-step ring: slots of a main and one helper wave
#define LWS_BUILD_tw_q6      lws::tw_q6,      "_r48",         0, 1, 1, 0, 0, 1, 6, 3    // 6 frames per row, 48-step ring
#define LWS_BUILD_tw_q8      lws::tw_q8,      "_r64",         0, 1, 1, 0, 0, 1, 0, 2    // the Q = 8 build's 64-step ring and helper waves with table twiddles

// The try order: a plan is served by the first of these whose systolic_build() accepts its shape and weights.
#define LWS_SYSTOLIC_BUILDS(X) \
    X(quarter_q2) X(quarter) X(half_q2) X(half) X(q2) X(narrow) X(q8) X(wide_q2) X(wide) X(xwide) X(l7) \
    X(tw_half) X(tw) X(tw_wide) X(tw_q5) X(tw_q6) X(tw_q8)

// LWS_ROW_FIELD(NS, half) -> lws::half, ...: the row becomes the argument list of the field's selector (this expands inside #if too)
#define LWS_ROW_FIELD(f, name) LWS_ROW_FIELD_(LWS_ROW_##f, name)
#define LWS_ROW_FIELD_(sel, name) LWS_ROW_APPLY(sel, LWS_BUILD_##name)
#define LWS_ROW_APPLY(sel, ...) sel(__VA_ARGS__)
#define LWS_ROW_NS(ns, tag, wide, q8, spw, l7, r16, tw, twq, slots) ns
#define LWS_ROW_TAG(ns, tag, wide, q8, spw, l7, r16, tw, twq, slots) tag
#define LWS_ROW_WIDE(ns, tag, wide, q8, spw, l7, r16, tw, twq, slots) wide
#define LWS_ROW_Q8(ns, tag, wide, q8, spw, l7, r16, tw, twq, slots) q8
#define LWS_ROW_SPW(ns, tag, wide, q8, spw, l7, r16, tw, twq, slots) spw
#define LWS_ROW_L7(ns, tag, wide, q8, spw, l7, r16, tw, twq, slots) l7
#define LWS_ROW_R16(ns, tag, wide, q8, spw, l7, r16, tw, twq, slots) r16
#define LWS_ROW_TW(ns, tag, wide, q8, spw, l7, r16, tw, twq, slots) tw
#define LWS_ROW_TWQ(ns, tag, wide, q8, spw, l7, r16, tw, twq, slots) twq
#define LWS_ROW_SLOTS(ns, tag, wide, q8, spw, l7, r16, tw, twq, slots) slots
