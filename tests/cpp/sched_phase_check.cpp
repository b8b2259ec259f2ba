// Host check of the schedule decision of option "reorder" (csrc/sched_phase.hpp, which rt_render's schedule step
// calls).  Usage: sched_phase_check table | sched_phase_check walk K
//   table   sched_step against the branch it replaced, restated below as it stood in rt_render, for layout_ok in
//           {0, 1}, K in 1..9 and every phase in 0..K-1: every output compared.  Prints {"cases", "mismatches"}.
//   walk K  3 K launches of one lane from a fresh layout, the lane's state kept as rt_render keeps it.  Prints
//           first_records_in_screen_order  launch 0 runs the schedule kernel without ordering, tracks, and traces
//                                          without an order
//           stale_orders                   launches that built an order although the costs it reads were not recorded
//                                          by an earlier launch of this layout (or the kernel had cleared them since)
//           orders_without_schedule        launches traced with an order no schedule kernel of this layout built
//           bad_periods                    K > 1: windows of K consecutive launches that do not hold exactly one
//                                          recording launch, or a recording launch whose successor does not order
//           records, orders                launches that tracked / that built an order
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../real-time-gpu-ray-tracer_amd/csrc/sched_phase.hpp"

using namespace rtamd;

// The branch as rt_render held it before sched_step, its lines unchanged between the markers (s->order_ok[q]: the lane's
// flag, ph: the lane's phase).
struct RefScene { bool order_ok[1]; };
static void reference(bool layout_ok, uint32_t K, uint32_t &ph, RefScene *s, bool &run_sched_out, bool &track_out, bool &do_order_out) {
    const int q = 0;
    // ---- rt_render, before ----
        bool run_sched, track;
        if (!layout_ok) {
            run_sched = true; track = true; s->order_ok[q] = false; ph = K == 1 ? 0u : 1u;
        } else if (K == 1) {
            run_sched = true; track = true;
        } else {
            run_sched = ph == 1; track = ph == 0; ph = (ph + 1) % K;
        }
        const bool do_order = layout_ok && run_sched;
    // ---- end ----
    run_sched_out = run_sched; track_out = track; do_order_out = do_order;
}

static int table() {
    unsigned cases = 0, mismatches = 0;
    for (int ok = 0; ok < 2; ok++)
        for (uint32_t K = 1; K <= 9; K++)
            for (uint32_t phase = 0; phase < K; phase++)
                for (int had_order = 0; had_order < 2; had_order++) {
                    uint32_t ph = phase;
                    RefScene ref{{had_order != 0}};
                    bool run_sched = false, track = false, do_order = false;
                    reference(ok != 0, K, ph, &ref, run_sched, track, do_order);
                    const bool order_ok = ref.order_ok[0];
                    const SchedStep d = sched_step(ok != 0, K, phase);
                    bool mine_order_ok = had_order != 0;
                    if (d.drop_order) mine_order_ok = false;
                    cases++;
                    if (d.run_sched != run_sched || d.track != track || d.do_order != do_order || d.phase != ph ||
                        mine_order_ok != order_ok || d.phase >= K)
                        mismatches++;
                }
    std::printf("{\"cases\": %u, \"mismatches\": %u}\n", cases, mismatches);
    return 0;
}

static int walk(uint32_t K) {
    // the lane as rt_render keeps it; a fresh layout: nothing valid, whatever phase and order the lane held before
    bool valid = false, order_ok = true;
    uint32_t phase = K - 1;
    bool costs_recorded = false;       // the cost buffer holds a whole launch's costs of this layout
    bool order_built = false;          // the order buffer holds an order built for this layout
    unsigned stale = 0, unscheduled = 0, records = 0, orders = 0;
    bool first_ok = false;
    std::vector<uint8_t> tracked, ordered;
    for (uint32_t i = 0; i < 3 * K; i++) {
        const SchedStep d = sched_step(valid, K, phase);
        phase = d.phase;
        if (d.drop_order) order_ok = false;
        if (d.run_sched) {
            if (d.do_order) {
                if (!costs_recorded) stale++;
                order_built = true;
                order_ok = true;
                orders++;
            }
            costs_recorded = false;    // the schedule kernel clears the costs it has read (or, without an order, all)
        }
        valid = true;
        if (order_ok && !order_built) unscheduled++;
        if (i == 0) first_ok = d.run_sched && !d.do_order && d.track && !order_ok;
        if (d.track) { costs_recorded = true; records++; }
        tracked.push_back(d.track);
        ordered.push_back(d.do_order);
    }
    unsigned bad_periods = 0;
    if (K > 1) {
        for (size_t i = 0; i + K <= tracked.size(); i++) {
            unsigned n = 0;
            for (uint32_t k = 0; k < K; k++) n += tracked[i + k];
            if (n != 1) bad_periods++;
        }
        for (size_t i = 0; i + 1 < tracked.size(); i++)
            if (tracked[i] && !ordered[i + 1]) bad_periods++;
    }
    std::printf("{\"first_records_in_screen_order\": %d, \"stale_orders\": %u, \"orders_without_schedule\": %u, "
                "\"bad_periods\": %u, \"records\": %u, \"orders\": %u}\n",
                first_ok ? 1 : 0, stale, unscheduled, bad_periods, records, orders);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && std::strcmp(argv[1], "table") == 0) return table();
    if (argc == 3 && std::strcmp(argv[1], "walk") == 0) {
        const long K = std::strtol(argv[2], nullptr, 10);
        if (K < 1 || K > 64) return 2;
        return walk((uint32_t)K);
    }
    return 2;
}
