// lws_switches.h -- the environment switches of the library (comparison runs, verification variants, the host pipeline's shape,
// test hooks): the one table of them and the one function that reads the environment.  What each switch does is told in
// INTEGRATION.md section 6, in this order.  Host-only C++17, no HIP header: the CPU tests compile it alone (tests/switches_main.cpp).
//
// A public entry point that can reach a launch or a geometry decision takes ONE snapshot (read_switches) into its plan; everything
// below it is handed the snapshot, or the one or two values it needs, and reads nothing itself.  No process-wide copy: tests change the
// environment between two calls of one plan, and lws_multi_* runs a plan per device on a thread each.
#pragma once

#include <climits>
#include <cstdlib>

// X(field, environment name, kind, default, binds)
//   kind   FLAG: on for any non-zero integer;  INT: the integer (atoi)
//   binds  CREATE: lws_plan_create reads it and what it decides stays with the plan;  CALL: every call reads it afresh
#define LWS_SWITCHES(X)                                                         \
    /* which engine takes a stage (lws_capi.hip: choose_engine) */              \
    X(team_first,            "LWS_TEAM_FIRST",            FLAG, 0,            CALL)   \
    X(team_fp64,             "LWS_TEAM_FP64",             FLAG, 0,            CALL)   \
    X(team_ordered,          "LWS_TEAM_ORDERED",          FLAG, 0,            CALL)   \
    X(no_team,               "LWS_NO_TEAM",               FLAG, 0,            CALL)   \
    X(no_team_q8,            "LWS_NO_TEAM_Q8",            FLAG, 0,            CALL)   \
    X(no_sys64,              "LWS_NO_SYS64",              FLAG, 0,            CALL)   \
    X(online64_one_wave,     "LWS_ONLINE64_ONE_WAVE",     FLAG, 0,            CALL)   \
    X(online_serial_taps,    "LWS_ONLINE_SERIAL_TAPS",    FLAG, 0,            CALL)   \
    X(nofuture_serial_taps,  "LWS_NOFUTURE_SERIAL_TAPS",  FLAG, 0,            CALL)   \
    /* which systolic build, which twiddles a plan gets (lws_plan_create) */    \
    X(no_systolic,           "LWS_NO_SYSTOLIC",           FLAG, 0,            CREATE) \
    X(systolic_no_short,     "LWS_SYSTOLIC_NO_SHORT",     FLAG, 0,            CREATE) \
    X(systolic_no_tw,        "LWS_SYSTOLIC_NO_TW",        FLAG, 0,            CREATE) \
    X(systolic_no_r16,       "LWS_SYSTOLIC_NO_R16",       FLAG, 0,            CREATE) \
    X(online_table_twiddles, "LWS_ONLINE_TABLE_TWIDDLES", FLAG, 0,            CREATE) \
    /* the host-array entry points of an fp32 plan (lws_capi.hip: run_host) */  \
    X(host_monolithic,       "LWS_HOST_MONOLITHIC",       FLAG, 0,            CALL)   \
    X(host_chunk_bins,       "LWS_HOST_CHUNK_BINS",       INT,  16 << 20,     CALL)   \
    X(host_chunk_exact,      "LWS_HOST_CHUNK_EXACT",      FLAG, 0,            CALL)   \
    X(host_pin_mb,           "LWS_HOST_PIN_MB",           INT,  2048,         CALL)   \
    X(host_half_first,       "LWS_HOST_HALF_FIRST",       FLAG, 1,            CALL)   \
    X(host_threads,          "LWS_HOST_THREADS",          INT,  SWITCH_UNSET, CALL)   \
    X(host_real,             "LWS_HOST_REAL",             FLAG, 1,            CALL)   \
    X(host_prefault,         "LWS_HOST_PREFAULT",         FLAG, 1,            CALL)   \
    X(host_trace,            "LWS_HOST_TRACE",            FLAG, 0,            CALL)   \
    /* the engines' own */                                                      \
    X(band_no_helpers,       "LWS_BAND_NO_HELPERS",       FLAG, 0,            CALL)   \
    X(band_skw,              "LWS_BAND_SKW",              INT,  0,            CALL)   \
    X(band_nls,              "LWS_BAND_NLS",              INT,  0,            CALL)   \
    X(band_ns,               "LWS_BAND_NS",               INT,  0,            CALL)   \
    X(band_chunk,            "LWS_BAND_CHUNK",            INT,  0,            CALL)   \
    X(online_lag_plus,       "LWS_ONLINE_LAG_PLUS",       INT,  0,            CALL)   \
    X(online_layout,         "LWS_ONLINE_LAYOUT",         INT,  0,            CALL)   \
    X(online64_stress,       "LWS_ONLINE64_STRESS",       INT,  0,            CALL)   \
    X(s64_chunk,             "LWS_S64_CHUNK",             INT,  1024,         CALL)   \
    X(team_lanes,            "LWS_TEAM_LANES",            INT,  0,            CALL)   \
    X(team_no_ring,          "LWS_TEAM_NO_RING",          FLAG, 0,            CALL)   \
    X(team_nch3,             "LWS_TEAM_NCH3",             FLAG, 0,            CALL)   \
    X(team_dbg_poison,       "LWS_TEAM_DBG_POISON",       FLAG, 0,            CALL)   \
    X(systolic_nwg,          "LWS_SYSTOLIC_NWG",          INT,  0,            CALL)   \
    X(systolic_spin_limit,   "LWS_SYSTOLIC_SPIN_LIMIT",   INT,  1 << 21,      CALL)   \
    X(systolic_stress,       "LWS_SYSTOLIC_STRESS",       INT,  0,            CALL)   \
    X(systolic_rolemap,      "LWS_SYSTOLIC_ROLEMAP",      INT,  0,            CALL)

namespace lws {

// LWS_HOST_THREADS has no constant default (its use site computes one from the plan and the CPUs): unset stays visible as this
constexpr int SWITCH_UNSET = INT_MIN;

enum class SwitchKind { FLAG, INT };
enum class SwitchWhen { CREATE, CALL };
namespace switch_detail { using FLAG = bool; using INT = int; }

struct Switches {
#define LWS_SWITCH_FIELD(field, name, kind, dflt, when) switch_detail::kind field = dflt;
    LWS_SWITCHES(LWS_SWITCH_FIELD)
#undef LWS_SWITCH_FIELD
};

// the table as data (tests/switches_main.cpp prints it)
struct SwitchRow { const char *name; SwitchKind kind; int dflt; SwitchWhen when; };
inline constexpr SwitchRow switch_rows[] = {
#define LWS_SWITCH_ROW(field, name, kind, dflt, when) {name, SwitchKind::kind, dflt, SwitchWhen::when},
    LWS_SWITCHES(LWS_SWITCH_ROW)
#undef LWS_SWITCH_ROW
};

// The environment, now: a variable that is unset or empty leaves the default.
inline Switches read_switches() {
    Switches s;
    const char *v;
#define LWS_SWITCH_READ(field, name, kind, dflt, when) if ((v = std::getenv(name)) && *v) s.field = static_cast<switch_detail::kind>(std::atoi(v));
    LWS_SWITCHES(LWS_SWITCH_READ)
#undef LWS_SWITCH_READ
    return s;
}

}  // namespace lws
