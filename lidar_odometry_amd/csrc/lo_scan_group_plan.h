// lo_scan_group_plan.h — scan groups: what the scan queue does with a scan that a caller queues behind others, decided
// from a snapshot like plan_scan's (lo_scan_plan.h) and nothing else.  No HIP here and no context: enqueue_optimize
// takes the snapshot (group_snapshot, lo_scanq.hip) and applies the plan, and tests/test_scan_group_plan.py runs the same
// function on a CPU against a simulated queue.
//
// A caller that queues scans back to back on one context hands the library a batch one scan at a time.  A groupable
// scan is not launched when it is enqueued: it is appended to the open group (its KParams and initial pose into the
// slot's pinned staging, its per-scan state one of the slot's sets), and the group leaves as one lockstep run
// (lo_lockstep.h) on the slot's stream -- when it is full, at every flush point (flush_hold), or at once when nothing of
// the context is in flight, so a lone asynchronous scan starts as it always did.  Two slots alternate: one group runs
// while the next fills.  A slot's stream orders a group behind the slot's previous one; the host waits only for the
// slot's previous uploads before it rewrites the staging (wait_staging), never for a group.
// Groupable: the scan would be pipelined and overlapped by plan_scan (a PKO candidate scan, not KDTree, nothing timed,
// caller-owned points, queue not flagged), is small enough for lockstep (fast mode, or exact with n <= merge_max), and
// no explicit choice asks for the ring: pipeline or overlap off, a chosen split or depth, the timeout test hook.  A
// context that is not alone in queueing scans keeps one scan in flight (plan_scan) and does not group either.
// Everything else yields: the open group is emitted first (record order is kept), then the scan takes the ring path.
#pragma once
#include "lo_scan_plan.h"

namespace lo {
constexpr int kGroupSlots = 2;
constexpr int kMaxGroup = 32;          // two groups fit the 64-record ring
constexpr int kDefaultGroup = 32;      // scans per group unless chosen (lo_set_scan_group / LO_SCAN_GROUP): measured,
                                       //   kitti queue 85.5 us per scan on the ring, 47.5 / 26.6 / 15.2 / 8.9 at 4 / 8 / 16 / 32
// A partial group of fewer scans than this goes down the ring one by one (emit_pipelined); a full group always runs in
// lockstep.  Measured (profiles/scan_group_batch_small.json): a lockstep run takes ~0.34 ms for 2 to 8 exact scans
// (0.25 ms fast), the ring ~0.086 ms per scan, so the two meet at 4 scans.
constexpr int kGroupLockstepMin = 5;

struct GroupPlanIn {
    ScanPlanIn scan;               // what plan_scan sees for this scan
    int group;                     // the setting: 0 default, 1 off, 2..kMaxGroup
    bool fail_hook;                // LO_PIPE_FAIL_AT is set: the ring's timeout test
    bool exact;                    // reference-exact mode
    int n;                         // the scan's points
    int merge_max;                 // lockstep limit of an exact job (kExactMergeMax)
    int open_n;                    // scans in the open group
    int open_slot;                 // the slot it fills
    bool in_flight;                // ring holds are pending, or an emitted group has not reported done
    bool staging_busy[kGroupSlots];   // the slot's last uploads have not been waited for
};

struct GroupPlan {
    int g;                         // scans per group in effect (1: grouping off)
    bool append;                   // the scan joins the open group; else the open group leaves and the scan yields
    bool emit;                     // the open group (with this scan, if appended) leaves now
    bool lockstep;                 //   as one lockstep run; else its scans one by one down the ring
    int slot;                      // the slot of the open group
    int next_slot;                 // the slot the next group fills
    bool wait_staging;             // the host waits for the slot's previous uploads before it writes this scan's staging
};

inline int group_size(int setting) { return setting == 0 ? kDefaultGroup : std::min(std::max(setting, 1), kMaxGroup); }

inline bool group_lockstep(int n, int g) { return n >= std::min(kGroupLockstepMin, g); }

// A flush point (flush_hold): the open group leaves whatever its size.
inline GroupPlan plan_group_flush(int open_n, int open_slot, int g) {
    GroupPlan p{};
    p.g = g;
    p.emit = open_n > 0;
    p.lockstep = group_lockstep(open_n, g);
    p.slot = open_slot;
    p.next_slot = (p.emit && p.lockstep) ? (open_slot + 1) % kGroupSlots : open_slot;
    return p;
}

inline GroupPlan plan_group(const GroupPlanIn& in) {
    GroupPlan p{};
    const ScanPlanIn& s = in.scan;
    p.g = group_size(in.group);
    const bool explicit_ring = !s.pipe || !s.overlap || !s.pipe_main_auto || !s.depth_auto || in.fail_hook;
    const bool ring_overlaps = s.cand && !s.kd && !s.timed && !s.stage_timing && !s.dev_count && !s.flagged;
    const bool small = !in.exact || in.n <= in.merge_max;
    p.append = p.g > 1 && !explicit_ring && s.others_holding == 0 && ring_overlaps && small && in.n > 0;
    p.slot = in.open_slot;
    if (!p.append) {                                   // the open group first, then the scan as it always went
        const GroupPlan f = plan_group_flush(in.open_n, in.open_slot, p.g);
        p.emit = f.emit;
        p.lockstep = f.lockstep;
        p.next_slot = f.next_slot;
        return p;
    }
    const int n = in.open_n + 1;
    p.wait_staging = in.open_n == 0 && in.staging_busy[in.open_slot];
    p.emit = n >= p.g || !in.in_flight;
    p.lockstep = group_lockstep(n, p.g);
    p.next_slot = (p.emit && p.lockstep) ? (in.open_slot + 1) % kGroupSlots : in.open_slot;
    return p;
}
}  // namespace lo
