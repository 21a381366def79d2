// vbs_schedule.h -- which bins of a variable-block-size batch share an order-search / K3 launch, in which
// order the launches are issued and which lane (stream) each goes to.  Pure host arithmetic: nothing from
// HIP, usable from a host-only compile (tests/test_vbs_schedule_cpu.py); api.hip walks the result.
#pragma once

namespace fhip {

constexpr int VBS_MAX_LANES = 5;        // the handle's stream (lane 0) and its four internal ones

// A bin's search + K3 is a launch's latency plus its live pieces' work, and the short pieces' bins hold more
// pieces (measured per 1024 blocks, eighths 1 .. 8, with three lanes busy: level 10 -- the vector searches --
// 175, 195, 192, 56, 54, 39, 72, 40 us; level 12 -- the matrix searches -- 275, 265, 245, 168, 137, 136, 115,
// 113): the weights are those, in units of 5 us.
inline const int *vbs_bin_weights(bool mat_search)
{
    static const int vec[8] = {35, 39, 38, 11, 11, 8, 14, 8}, mat[8] = {55, 53, 49, 34, 27, 27, 23, 23};
    return mat_search ? mat : vec;
}

// The lane a unit's launches go to: the one with the least estimated work queued (the first of equals).
inline int vbs_take_lane(long long *queued, int nlanes, int weight)
{
    int h = 0;
    for (int q = 1; q < nlanes; q++) if (queued[q] < queued[h]) h = q;
    queued[h] += weight;
    return h;
}

struct VbsUnit { int nbins, bins[8], weight, lane; };     // bins ascending; one member: the per-bin launchers
struct VbsSchedule {
    int nunits;
    VbsUnit unit[8];          // in issue order: heaviest first
    int lane_of[8];           // per bin: its unit's lane (0 = the handle's stream)
};

// key[k] >= 0: bin k may share a launch with the other bins of that key (the caller decides: the thinly filled
// bins of a small batch, four eighths and longer, by the kernel they can share); -1: a launch of its own.
// fan false (serial, or profiling): everything on lane 0, the order of issue unchanged.
inline VbsSchedule vbs_schedule(const int key[8], bool mat_search, bool fan, int nlanes)
{
    const int *bin_weight = vbs_bin_weights(mat_search);
    int unit_of[8], unit_w[8] = {0}, nunits = 0;
    for (int k = 0; k < 8; k++) {
        unit_of[k] = -1;
        for (int q = 3; q < k && key[k] >= 0; q++) if (key[q] == key[k]) { unit_of[k] = unit_of[q]; break; }
        if (unit_of[k] < 0) unit_of[k] = nunits++;
        // (a group costs its first member's latency once: 95 us of three launches were 55 in one)
        unit_w[unit_of[k]] += (unit_w[unit_of[k]] > 0) ? 2 : bin_weight[k];
    }
    VbsSchedule s{};
    s.nunits = nunits;
    long long queued[VBS_MAX_LANES] = {0};
    bool done[8] = {false};
    for (int turn = 0; turn < nunits; turn++) {
        int u = -1;
        for (int q = 0; q < nunits; q++) if (!done[q] && (u < 0 || unit_w[q] > unit_w[u])) u = q;
        done[u] = true;
        VbsUnit &un = s.unit[turn];
        un.weight = unit_w[u];
        un.lane = fan ? vbs_take_lane(queued, nlanes, unit_w[u]) : 0;
        for (int k = 0; k < 8; k++) if (unit_of[k] == u) { un.bins[un.nbins++] = k; s.lane_of[k] = un.lane; }
    }
    return s;
}

}  // namespace fhip
