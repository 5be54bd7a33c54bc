// lo_scan_plan.h — what the scan queue does with one scan, decided from a snapshot of the queue's state and nothing
// else.  No HIP here and no context: enqueue_optimize takes the snapshot (scan_snapshot, lo_scanq.hip), calls plan_scan,
// applies the plan (apply_plan) and emits the launches (emit_pipelined), and tests/test_scan_plan.py runs the same
// function on a CPU against a simulated queue.
//
// The queue.  A small PKO scan that nothing times is "pipelined": its GN iterations below the split run on the context
// stream, the rest (the tail) on a lane stream behind a device-side wait for the main part (k_wait_seq), and the context
// stream is held (k_wait_final, "the hold") only until the scan's result is final.  With scan overlap the hold is not
// enqueued with its scan but kept pending and placed by a later scan, so that scan's head (first correspondence launch
// + exact scale) runs beside this scan's tail.  The head rewrites per-scan state the tail still reads, so a context
// has up to kMaxLanes sets of it (lanes), and up to `depth` scans in flight, scan k of a queue on lane k % max(depth, 2).
//
// Host submission order of a queue of scans with d = depth >= 2 in flight, scan k on lane k % d:
//   context stream:     k_wait_final(k - d) -> head(k) -> main(k)     (the wait: pops_before_head)
//   lane stream k % d:  k_wait_seq(k) -> tail(k)
// and k_wait_final(k) is placed by scan k + d, or by flush_hold.  main(k) is the iterations below the split: with split
// 0 (the queue's split from three in flight on) there is none, the context stream carries k_wait_final(k - d) ->
// head(k) -> k_signal_main(k), and every iteration is tail(k).  With one scan in flight (depth 1) the context stream
// carries head(k) -> k_wait_final(k - 1) -> main(k) instead (flush_after_head), and every tail shares lane stream 0:
// tail(k) starts behind tail(k - 1) anyway, and a third stream per context only crowds the hardware queues of a process
// that runs many contexts.
// Every device-side wait depends only on work submitted before it, on any stream: k_wait_final(j) polls the lane's word
// that main(j) or tail(j) publishes, both submitted during scan j's own call, which returned before any call that can
// place that wait; k_wait_seq(k) polls the lane's word that main(k)'s last pick sets -- with split 0 the one
// k_signal_main(k) sets behind head(k) -- submitted just above it, or the one main(k) publishes when it ends the scan.
// Nothing waits for a later submission, so the order is deadlock-free even if all the streams share one hardware queue
// (they then simply run in this order), and every wait is bounded by the queue's wait bound besides.
// head(k) rewrites the lane state of scan k - d: k_wait_final(k - d) precedes it on this stream, so that scan is final,
// and what is left of its tail leaves on tail_gone before touching anything.  The lane's words count the lane's own
// scans, which are final in order; between the lanes no order is assumed -- scan k may be final before scan k - 1.
// main(k) and main(k - 1) follow each other on the context stream; with split 0 tail(k) and tail(k - 1) share nothing
// but the map and the tables, which neither writes.
#pragma once
#include <algorithm>

namespace lo {
constexpr int kMaxLanes = 4;       // sets of per-scan state, and queued scans in flight at most (scan ring)
constexpr int kDefaultDepth = 4;   // queued scans in flight unless chosen: 4 with split 0 measured +27 % over 2, and 3
                                   //   only +2 % (DESIGN.md "Scan ring")

struct ScanPlanIn {                // read-only snapshot of the queue and of the scan being enqueued
    int depth, depth_used;         // scans in flight as set, and the depth the pending holds were placed for
    bool depth_auto;               // no depth chosen
    int others_holding;            // other contexts of the process with queued scans in flight right now
    bool pipe, overlap;
    int pipe_main;                 // the split as set
    bool pipe_main_auto;           //   no split chosen
    int lane, n_hold;
    int hold_lane[kMaxLanes];      // the pending holds' lanes, oldest first
    bool cand, kd;                 // the scan pre-solves candidates (cand_scan); a KDTree context
    bool timed, stage_timing;      // HIP events or the stage timing bracket the whole scan
    bool dev_count;                // a device-filtered scan: it sits in the context's one point buffer, which the next
                                   //   raw call's filter overwrites, so that call enqueues the hold first anyway
    bool flagged;                  // an earlier scan's wait timed out (the caller recovers: one stream from now on)
    int max_iterations;
};

struct ScanPlan {
    int depth;                     // scans in flight for this scan
    bool flush_before;             // every pending hold out first: the depth changed, or this scan does not overlap
    bool overlaps;                 // its head goes in front of a pending hold, on the next lane of the ring
    int lane;                      // the lane it runs on (after the switch, if it overlaps)
    int pops_before_head;          // oldest holds enqueued in front of the head (depth >= 2)
    bool pipelined;
    int split;                     // iterations < split on the context stream, the rest on the tail stream
    bool signal_main;              // split 0: "head done" is a launch of its own behind the head
    bool flush_after_head;         // depth 1: the one pending hold, behind this scan's head
    int tail_stream;               // which lane's stream carries the tail
    bool push_hold;                // the scan's own hold stays pending; else k_wait_final at once
};

inline ScanPlan plan_scan(const ScanPlanIn& in) {
    ScanPlan p{};
    // Two or more in flight pay while the chip is half idle under one context's queue; when other contexts of the
    // process are queueing scans too, their launches already fill it, and a second scan in flight per context only adds
    // waits to the few hardware queues all their streams share (8 contexts: 24 streams on 4 queues ran 31 % slower in
    // aggregate).  So unless a depth was chosen, a context that is not alone in having scans in flight keeps one.
    p.depth = (in.depth_auto && in.others_holding > 0) ? 1 : in.depth;
    // (holds placed for another depth were placed for another order: all out first, none left to overlap with)
    const int n_hold = p.depth != in.depth_used ? 0 : in.n_hold;
    // A hold may be deferred (and a deferred one kept past this scan's head) only between two pipelined scans that
    // nothing times and whose points are the caller's.
    const bool may_defer = in.overlap && !in.timed && !in.stage_timing && !in.dev_count && !in.flagged;
    const bool pipe_ok = in.cand && !in.kd && in.pipe;
    // This scan's head overlaps: a hold is pending and the scan is pipelined.  Only then does it take the queue's split
    // (1 by default): the caller is queueing scans back to back, and the next head hides under a longer tail.  A scan
    // behind a flushed hold keeps the split 2 a scan always had unless one was chosen -- split 1 without overlap costs
    // about 1 %.  Three or more in flight and no split chosen: the queue's split is 0 -- every GN iteration of an
    // overlapping scan runs on its lane's stream, and the context stream carries only the heads and the holds.
    const int queue_split = (in.pipe_main_auto && p.depth >= 3) ? 0 : in.pipe_main;
    p.overlaps = n_hold != 0 && may_defer && pipe_ok && in.max_iterations > queue_split;
    p.split = (in.pipe_main_auto && !p.overlaps) ? 2 : queue_split;
    p.pipelined = pipe_ok && !in.flagged && in.max_iterations > p.split;
    p.signal_main = p.split == 0;
    p.flush_before = in.n_hold != 0 && !p.overlaps;
    p.lane = in.lane;
    int left = 0;                  // holds still pending when this scan's own would be pushed
    if (p.overlaps) {
        // the next lane of the ring, which scan k - depth used.  Two or more in flight: that scan's hold may still be
        // pending (with every older one), and goes in front of this scan's head, which rewrites the state its tail
        // reads.  Never more than `depth` in flight either, whatever lanes an earlier depth left the holds on.
        p.lane = (in.lane + 1) % std::max(p.depth, 2);
        if (p.depth > 1) {
            int pops = std::max(n_hold - p.depth + 1, 0);
            for (int i = 0; i < n_hold; ++i)
                if (in.hold_lane[i] == p.lane) pops = std::max(pops, i + 1);
            p.pops_before_head = pops;
            left = n_hold - pops;
        } else {
            p.flush_after_head = true;
        }
    }
    p.tail_stream = p.depth > 1 ? p.lane : 0;
    p.push_hold = may_defer && p.pipelined && left < kMaxLanes;
    return p;
}
}  // namespace lo
