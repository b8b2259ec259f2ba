// sched_phase.hpp — option "reorder": what a lane's launch does with its unit costs.  Shared by rt_render's schedule
// step (render.cpp) and the host check that pins it (tests/cpp/sched_phase_check.cpp), so the header is plain C++
// without HIP types.
//
// A lane records unit costs on one launch in K ("reorder_period") and rebuilds its claim order from them on the next;
// the launches between reuse the order.  Phase 0 records, phase 1 orders; K = 1: both on every launch.  A new layout
// (the costs the lane's previous launch recorded are for the layout it had) starts over: the schedule kernel clears
// the costs, the order is dropped, and this launch records in screen order.
#pragma once

#include <stdint.h>

namespace rtamd {

struct SchedStep {
    bool run_sched;     // the schedule kernel runs in front of this launch
    bool track;         // this launch records its unit costs
    bool do_order;      // the schedule kernel builds the order from the recorded costs (else it clears them)
    bool drop_order;    // the lane's order belongs to another layout: order_ok is cleared
    uint32_t phase;     // the lane's phase after this launch
};

// layout_ok: the lane's recorded costs belong to this launch's layout; phase < K, the lane's phase before the launch
inline SchedStep sched_step(bool layout_ok, uint32_t K, uint32_t phase) {
    if (!layout_ok) return {true, true, false, true, K == 1 ? 0u : 1u};
    if (K == 1) return {true, true, true, false, phase};
    return {phase == 1, phase == 0, phase == 1, false, (phase + 1) % K};
}

}  // namespace rtamd
