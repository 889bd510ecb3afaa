// lws_online.h -- LDS-resident fp32 engine for the online driver (lws_online.hip).  Internal, not part of the ABI.
#pragma once
#include "lws_common.h"

namespace lws {

// How a stage runs on this engine (online_plan): the layout -- 2: k_online, 2Q lanes per bin; 4: k_online4, one wave per tap group --
// and that kernel's launch parameters.  ok == false: the caller uses another engine.
struct OnlinePlan {
    int layout;             // 2 or 4
    int NSW, DS;            // sweep slots; steps between consecutive sweeps
    int threads;
    size_t lds;             // dynamic LDS, bytes
    int NWR, NPS;           // layout 4: frames in the LDS ring, its row stride
    bool big;               // layout 4: the variant for long frames (target magnitudes stay in the caller's buffer)
    bool serial;            // LWS_ONLINE_SERIAL_TAPS=1: the verification variant (the generic engine's bits)
    bool table;             // twiddles from the plan's table (layout 4 only) instead of static eighth turns
    bool ok;
};
// Plans a stage, once: ok if launch_online_lds can run this shape -- all three tensors with the common twiddle structure (tw_P, tw_s) that
// WeightStructure::twiddle (lws_weights.h) finds -- static eighth turns (P = Q in {2,4,8}, s = 1: either layout) or a table (Q in 3..8, any P <= 512:
// layout 4) -- L <= 5 (L = 5 for layout 2), the window of frames the sweeps in flight need fits the LDS ring.  Of the call's
// switches `sw` it uses LWS_ONLINE_SERIAL_TAPS, LWS_ONLINE_LAG_PLUS, LWS_ONLINE_LAYOUT; the launcher uses none.
OnlinePlan online_plan(const Switches &sw, int F, int T, int L, int Q, int Qp, int LA, int n_thr, int update, int tw_P, int tw_s, bool table);
// [P + 3][TQ] complex twiddles for the table variant, TQ = 4 (Q <= 4) or 8 (out: 2 (P + 3) TQ floats)
void online_twiddle_table(int P, int s, int Q, float *out);
// do the twiddles exp(2 pi j p r s / P) need no table (eighth turns of Q in {2,4,8})?  force_table: LWS_ONLINE_TABLE_TWIDDLES at plan creation
bool online_static_twiddles(int Q, int tw_P, int tw_s, bool force_table);

// Same contract as launch_generic<float> with mode == MODE_ONLINE, as online_plan planned it for this shape.  tw_table_dev: the uploaded
// online_twiddle_table (table variant: tw_P is its period), else null
hipError_t launch_online_lds(const OnlinePlan &pl, const GenericArgs<float> &a, int B, int tw_P, const float *tw_table_dev, hipStream_t stream);

}  // namespace lws
