// lo_scanq.h — the scan queue's state (lo_ctx::q) and the lanes of per-scan device state it switches between.  Its
// functions are in lo_scanq.hip; what it does with a scan is decided in lo_scan_plan.h, which also argues the order.
#pragma once
#include <cstdint>

#include "lo_buf.h"
#include "lo_device.h"
#include "lo_scan_group_plan.h"
#include "lo_scan_plan.h"

namespace lo {
constexpr int kFinWords = 4;                          // fence words per lane (ScanQueue::d_fin; pipe_fail relies on the 4)
static_assert(kMaxLanes == kFinLanes && kFinWords == 4, "pipe_fail masks a fence-word address to the block of all lanes");
constexpr int kRingRecords = 64;                      // lo_icp_queue_records: records kept per context
constexpr int kRecWords = 16;                         //   floats per record (lo_icp_export_pose's layout)

// One set of the state a scan's launches write and its tail still reads while the next scan's head runs.
struct ScanLane {
    DevBuf<int32_t> d_slot;
    DevBuf<double> d_res_pko;       // per-point residual of the accepted correspondences (the PKO sample reads it)
    DevBuf<uint64_t> d_wmask;
    DevBuf<int32_t> d_blk_cnt;
    DevBuf<double> d_blk_sum, d_blk_m2, d_blk_part;
    DevBuf<double> d_js;
    DevBuf<DevState> d_st;
    DevBuf<double> d_acc_part;      // speculative normal equations (lane_alloc_cand)
    DevBuf<float> d_cand_rec;       //   and each candidate's solved GN step [NA + 1][kCandWords]
    DevBuf<unsigned> d_cand_cnt;    //   per-candidate workgroup arrivals (zero between launches)
};

// Scan groups (lo_scan_group_plan.h; lo_set_scan_group / LO_SCAN_GROUP): queued scans that leave as lockstep runs.
// A slot is one group's worth of everything such a run owns: a stream, up to kMaxGroup sets of per-scan state (made the
// first time a scan uses them, without the speculative candidate buffers, which a lockstep run never touches), and the
// pinned staging and device copies of the jobs' KParams and initial poses.
constexpr int kGroupPkoWGs = 256;   // PKO workgroups per launch over all jobs of a group (>= 1 per job)
struct GroupJob {                   // one scan of the open group, as it was enqueued
    const float* pts;
    int n;
    float T0[12];
    bool exact;
    KParams P;                      // as make_params built it on the scan's own set of per-scan state
};
struct GroupSlot {
    hipStream_t s = nullptr;
    ScanLane sets[kMaxGroup];
    int n_sets = 0;                 // sets allocated so far (the first n_sets)
    PinnedBuf<KParams> h_Ps;        // the jobs' params in lockstep order (fast jobs, then exact ones): what is uploaded
    DevBuf<KParams> d_P;
    PinnedBuf<float> h_T0;          // sorted order
    DevBuf<float> d_T0;
    hipEvent_t ev_up = nullptr;     // behind the slot's last uploads: the host waits for it before rewriting the staging
    bool up_pending = false;
    hipEvent_t ev_done = nullptr;   // behind the slot's last group (flush_hold: the context stream waits for it)
    bool unjoined = false;          //   the context stream has not yet been made to wait for the slot's last group
    uint32_t seq = 0;               // groups emitted on this slot; the group's export kernel stores it to h_done[slot]
};
struct ScanGroups {
    int setting = 0;                // lo_set_scan_group: 0 default, 1 off, 2..kMaxGroup
    bool ready = false;             // streams, events, staging and the completion words exist
    GroupSlot slot[kGroupSlots];
    int open_slot = 0;
    int open_n = 0;                 // scans appended to the open group
    GroupJob jobs[kMaxGroup];
    ScanLane* cur = nullptr;        // the per-scan state of the last enqueued scan when that was a grouped one (cur(c))
    ScanLane* prev = nullptr;       //   and of the grouped scan enqueued before it (lo_debug_other_lane_record)
    MappedBuf<uint32_t> h_done;     // device-mapped, one word per slot: the last group of the slot that has finished
    uint32_t* d_hdone = nullptr;    //   its device alias (not owned)
    hipEvent_t ev_ring = nullptr;   // behind the ring's holds on the context stream, when a group follows ring scans
    int pko_budget = kGroupPkoWGs;  // PKO workgroups per launch over a group's jobs (LO_SCAN_GROUP_PKO_WGS)
    bool active = false;            // this context counts among those with queued scans in flight (holds pending, an
                                    //   open group, or a group the context stream has not been made to wait for)
    unsigned long long n_groups = 0, n_scans = 0;   // lockstep groups emitted, and scans they carried (lo_scan_group_status)
    bool in_flight() const {
        for (int i = 0; i < kGroupSlots; ++i)
            if (slot[i].seq != 0 && __atomic_load_n(h_done.get() + i, __ATOMIC_ACQUIRE) != slot[i].seq) return true;
        return false;
    }
};

// Scan pipeline (lo_set_pipeline; on by default): GN iterations >= the split of a small PKO scan go to a tail stream,
// and the context stream is held (k_wait_final) only until the scan's result is final -- a converged scan's early-exit
// launches drain beside the next scan instead of in front of it.  The tail starts when the main part is done (k_wait_seq
// polls the word the main part's last pick sets); no HIP events on the hot path (every marker packet costs ~5-7 us of
// device time between two kernels).
// Scan overlap (lo_set_scan_overlap; on by default, LO_OVERLAP=0): a pipelined scan does not end with its k_wait_final
// -- the hold stays pending in `holds` and is enqueued by a later pipelined scan, whose head therefore runs beside this
// scan's tail.  The head writes the per-scan state the tail still reads, so the queue owns up to kMaxLanes sets of it:
// `lanes[lane]` is the current one (cur(c); every launch's KParams name its buffers), lane_switch makes another one
// current.  Lane 0's base set is made with the context and its candidate buffers by the first PKO optimize; any other
// lane is allocated whole the first time a scan runs there, so a context that never queues scans pays for none (~1.5 MB
// each at the default max_points).  Every other entry point that touches the context stream or a queued scan's inputs
// enqueues the pending holds first (flush_hold), after which the context is as if none of this existed.  The map and
// the PKO tables are shared; each lane has its own fence words and tail stream.
// `depth` scans in flight (lo_set_scan_depth / lo_set_scan_lanes / LO_OVERLAP_DEPTH), scan k of a queue on lane
// k % max(depth, 2): from 2 on, the hold of scan k - 1 is no longer enqueued by scan k, only the hold of scan k - depth
// -- the scan that last used scan k's lane -- and in front of scan k's head.  So up to `depth` holds are pending, and
// scan k's GN iterations run beside scan k - 1's tail.
struct ScanQueue {
    bool pipe = true;
    int pipe_main = 1;              // the split of a scan whose head overlapped (1: the tail then carries ~1.4 working
                                    //   iterations per scan, and the whole head of the next scan hides under it)
    bool pipe_main_auto = true;     // no split chosen (lo_set_pipeline / LO_PIPE_MAIN): plan_scan picks 2, pipe_main or 0
    bool overlap = true;
    int depth = kDefaultDepth;
    bool depth_auto = true;         // no depth chosen: one scan in flight while other contexts queue scans too (plan_scan)
    int depth_used = kDefaultDepth; // the depth the pending holds were placed for
    ScanLane lanes[kMaxLanes];
    bool lane_ready[kMaxLanes] = {true, false, false, false};   // lane i has a full set, its candidate buffers sized for
                                    //   the current alpha grid (lane 0: those come with the first PKO optimize)
    int lane = 0;                   // the current lane
    int prev_lane = -1;             // the lane the last switch left: the scan enqueued before the last one ran there
                                    //   (lo_debug_other_lane_record; -1: no scan has overlapped yet)
    hipStream_t s_tail[kMaxLanes] = {};   // one tail stream per lane, made when a scan's tail first runs there
    struct Hold {
        uint32_t seq;               // the scan's number on its lane
        int lane;
        DevState* st;               // its lane's DevState (a timed-out wait marks it LO_ERR_PIPELINE)
    };
    Hold holds[kMaxLanes];          // the scans whose k_wait_final is still to be enqueued, oldest first
    int n_hold = 0;
    uint32_t pipe_seq = 0;          // pipelined scans so far (LO_PIPE_FAIL_AT counts in it)
    uint32_t lane_seq[kMaxLanes] = {};   // each lane's own sequence number: what its fence words count in (never 0)
    DevBuf<uint32_t> d_fin;         // kFinWords per lane, kMaxLanes groups (KParams::fin names the lane's group): [0] the
                                    // lane's last scan whose result is final (publish_final), [1] main part done, [2]
                                    // signal_main's block count, [3] broken (a wait timed out; sticky, and set in every
                                    // group: pipe_fail)
    MappedBuf<uint32_t> h_broken;   // device-mapped: the seq of the scan whose wait timed out (0: none)
    uint32_t* d_hbroken = nullptr;  //   its device alias (not owned)
    unsigned long long pipe_bound = 200000000ull;   // wait bound in 100 MHz ticks (2 s; LO_PIPE_WAIT_MS)
    uint32_t pipe_fail_at = 0;      // test hook (LO_PIPE_FAIL_AT=k): the k-th pipelined scan's tail wait gives up at once
    unsigned pipe_timeouts = 0;     // times a wait timed out and the pipeline was switched off (lo_pipeline_status)
    unsigned pipe_reruns = 0;       // synchronous scans re-run on one stream after such a timeout
    // every pipelined scan's 16-float record (lo_icp_queue_records): the thread that publishes a scan final writes it
    DevBuf<float> d_ring;           // kRingRecords x kRecWords floats
    unsigned long long ring_pos = 0;   // pipelined scans given a slot so far (slot = ring_pos % kRingRecords)
    unsigned ring_n = 0;            // of which the last ring_n were queued with no other scan in between (<= kRingRecords)
    unsigned long long overlapped = 0;   // scans whose head was enqueued in front of the previous scan's hold
    ScanGroups grp;                 // scan groups (above)

    void from_env();                // LO_PIPE, LO_PIPE_MAIN, LO_OVERLAP, LO_OVERLAP_DEPTH, LO_PIPE_WAIT_MS, LO_PIPE_FAIL_AT,
                                    //   LO_SCAN_GROUP
    bool flagged() const { return h_broken && __atomic_load_n(h_broken.get(), __ATOMIC_ACQUIRE) != 0u; }
};
}  // namespace lo
