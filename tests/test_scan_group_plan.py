"""plan_group (csrc/lo_scan_group_plan.h), the scan queue's decision for one queued scan, on the host alone.

A stand-alone C++ program includes the header (no HIP) and simulates a queue the way enqueue_optimize, group_append,
group_emit and flush_hold apply the plan: the open group and its slot, which slots' uploads and groups are marked in
flight, and the ring's pending holds.  It checks that no group exceeds G, that the open group leaves at every kind of
flush, that every explicit choice of the ring (and every scan that is not groupable) yields to the ring with the open
group sent first, that the slots alternate, and that a slot's staging is never rewritten while its last uploads are
marked in flight without the plan asking for the wait.  A slot whose previous GROUP is still marked in flight is reused
on purpose -- the slot's stream orders the new group behind the old one's export -- so the simulation keeps that mark
only to tell whether anything is in flight; what must never be reused early is the host staging, and that is checked -- over fixed sequences and a few thousand random ones (fixed
seed).  The program exits with the line number of the first check that fails.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_odometry_amd", "csrc")

SOURCE = r"""
#include "lo_scan_group_plan.h"

#include <cstdint>
#include <cstdio>

using namespace lo;

#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); return __LINE__; } } while (0)

struct Sim {
    GroupPlanIn in{};
    bool group_busy[kGroupSlots] = {};   // a group is marked in flight on the slot (until done())
    int emitted = 0, largest = 0, ring_scans = 0, last_slot = -1;
    int bad_staging = 0, bad_alternation = 0, over = 0;

    Sim() {
        ScanPlanIn& s = in.scan;
        s.depth = s.depth_used = kDefaultDepth;
        s.depth_auto = true;
        s.pipe = s.overlap = true;
        s.pipe_main = 1;
        s.pipe_main_auto = true;
        s.cand = true;
        s.max_iterations = 4;
        in.n = 500;
        in.merge_max = 8192;
        in.exact = true;
    }
    void emit(const GroupPlan& p, int n) {
        if (!p.lockstep) {                  // scan by scan down the ring: holds pending from here on
            ring_scans += n;
            in.scan.n_hold = 1;
        } else {
            ++emitted;
            if (n > largest) largest = n;
            if (n > group_size(in.group)) ++over;
            if (last_slot >= 0 && p.slot == last_slot) ++bad_alternation;
            last_slot = p.slot;
            in.scan.n_hold = 0;             // (the ring's holds go first)
            in.staging_busy[p.slot] = true;
            group_busy[p.slot] = true;
        }
        in.open_n = 0;
        in.open_slot = p.next_slot;
        refresh();
    }
    void refresh() { in.in_flight = in.scan.n_hold > 0 || group_busy[0] || group_busy[1]; }
    void done() { group_busy[0] = group_busy[1] = false; in.scan.n_hold = 0; refresh(); }   // the device caught up
    void flush() {                          // flush_hold
        const GroupPlan p = plan_group_flush(in.open_n, in.open_slot, group_size(in.group));
        if (p.emit) emit(p, in.open_n);
        in.scan.n_hold = 0;
        refresh();
    }
    GroupPlan scan() {
        const GroupPlan p = plan_group(in);
        if (p.append && (p.lockstep || !p.emit)) {
            if (in.open_n == 0 && in.staging_busy[in.open_slot] && !p.wait_staging) ++bad_staging;
            if (p.wait_staging) in.staging_busy[in.open_slot] = false;
            ++in.open_n;
            if (p.emit) emit(p, in.open_n);
            return p;
        }
        if (in.open_n > 0) {
            const GroupPlan f = plan_group_flush(in.open_n, in.open_slot, group_size(in.group));
            emit(f, in.open_n);
        }
        ++ring_scans;                       // the scan itself, down the ring
        in.scan.n_hold = (in.scan.timed || !in.scan.cand) ? 0 : 1;
        refresh();
        return p;
    }
};

static int sequences() {
    for (int g : {0, 2, 4, 8, 16, 32}) {   // a long queue: one ring scan, then full groups on alternating slots
        Sim q;
        q.in.group = g;
        const int G = group_size(g);
        CHECK(G == (g == 0 ? kDefaultGroup : g) && G <= kMaxGroup);
        GroupPlan p = q.scan();
        CHECK(p.append && p.emit && !p.lockstep && q.ring_scans == 1 && q.in.open_n == 0);   // idle: at once, the ring
        for (int k = 0; k < 5 * G; ++k) {
            p = q.scan();
            CHECK(p.append && p.emit == ((k + 1) % G == 0));
            if (p.emit) CHECK(p.lockstep && p.slot == (k / G) % kGroupSlots && p.next_slot == (k / G + 1) % kGroupSlots);
            CHECK(p.wait_staging == (k % G == 0 && k / G >= kGroupSlots));     // a slot's third use on
        }
        CHECK(q.emitted == 5 && q.largest == G && q.over == 0 && q.bad_alternation == 0 && q.bad_staging == 0);
        if (G >= 8) {
            for (int k = 0; k < kGroupLockstepMin; ++k) q.scan();
            CHECK(q.in.open_n == kGroupLockstepMin);
            q.flush();                      // a partial group leaves at a flush
            CHECK(q.in.open_n == 0 && q.emitted == 6 && q.bad_alternation == 0);
            const int rs = q.ring_scans;
            for (int k = 0; k < kGroupLockstepMin - 1; ++k) q.scan();
            q.flush();                      // ... and a smaller one goes down the ring scan by scan
            CHECK(q.emitted == 6 && q.ring_scans == rs + kGroupLockstepMin - 1);
        }
        q.done();
        p = q.scan();                       // nothing in flight again: at once
        CHECK(p.append && p.emit && !p.lockstep);
    }
    {   // group 1: every scan yields
        Sim q;
        q.in.group = 1;
        for (int k = 0; k < 9; ++k) { const GroupPlan p = q.scan(); CHECK(!p.append && !p.emit && p.g == 1); }
        CHECK(q.emitted == 0 && q.ring_scans == 9);
    }
    // every explicit choice of the ring, and every scan that is not groupable: the open group first, then the ring
    for (int knob = 0; knob < 14; ++knob) {
        Sim q;
        q.in.group = 4;
        q.scan(); q.scan(); q.scan();
        CHECK(q.in.open_n == 2 && q.emitted == 0);
        ScanPlanIn& s = q.in.scan;
        switch (knob) {
            case 0: s.pipe = false; break;
            case 1: s.overlap = false; break;
            case 2: s.pipe_main_auto = false; break;
            case 3: s.depth_auto = false; break;
            case 4: q.in.fail_hook = true; break;
            case 5: s.others_holding = 1; break;
            case 6: s.cand = false; break;
            case 7: s.kd = true; break;
            case 8: s.timed = true; break;
            case 9: s.stage_timing = true; break;
            case 10: s.dev_count = true; break;
            case 11: s.flagged = true; break;
            case 12: q.in.n = 8193; break;           // exact, beyond the lockstep limit
            case 13: q.in.n = 0; break;
        }
        const GroupPlan p = q.scan();
        CHECK(!p.append && p.emit && !p.lockstep);   // (two scans: below kGroupLockstepMin, down the ring)
        CHECK(q.emitted == 0 && q.in.open_n == 0 && q.ring_scans == 4);
    }
    {   // fast mode has no size limit of its own (cand bounds it)
        Sim q;
        q.in.group = 4;
        q.in.exact = false;
        q.in.n = 16000;
        q.scan();
        CHECK(q.scan().append);
    }
    return 0;
}

static uint32_t rng_state = 12345u;
static uint32_t rnd(uint32_t n) { rng_state = rng_state * 1664525u + 1013904223u; return (rng_state >> 8) % n; }

static int random_walk() {
    for (int run = 0; run < 300; ++run) {
        Sim q;
        q.in.group = static_cast<int>(rnd(34));             // 0 .. 33: beyond kMaxGroup is clamped
        if (q.in.group > kMaxGroup) q.in.group = kMaxGroup;
        for (int step = 0; step < 200; ++step) {
            const uint32_t r = rnd(100);
            ScanPlanIn& s = q.in.scan;
            if (r < 4) q.flush();
            else if (r < 8) q.done();
            else if (r < 10) { q.flush(); s.depth_auto = !s.depth_auto; }      // the setters flush first
            else if (r < 12) { q.flush(); s.overlap = !s.overlap; }
            else if (r < 14) { q.flush(); q.in.exact = !q.in.exact; }
            else {
                s.timed = rnd(40) == 0;
                s.cand = rnd(30) != 0;
                q.in.n = rnd(25) == 0 ? 9000 : 500;
                const int open = q.in.open_n;
                const GroupPlan p = q.scan();
                if (!p.append) CHECK(q.in.open_n == 0);     // whatever was open went out first
                else CHECK(q.in.open_n == (p.emit ? 0 : open + 1));
                CHECK(q.in.open_n < group_size(q.in.group) || group_size(q.in.group) == 1);
            }
            CHECK(q.over == 0 && q.bad_staging == 0 && q.bad_alternation == 0 && q.largest <= kMaxGroup);
        }
        q.flush();
        CHECK(q.in.open_n == 0);
    }
    return 0;
}

int main() {
    if (int rc = sequences()) return rc;
    if (int rc = random_walk()) return rc;
    std::printf("ok\n");
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None and shutil.which("c++") is None, reason="no host C++ compiler")
def test_plan_group_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    src = tmp_path / "plan_group.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "plan_group"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-I", CSRC, str(src),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
