// Row ranges ("lanes") of a launch-path decode: contiguous row ranges of the batch, each on its own HIP stream with its own step state, so that
// the latency chains of one range's small kernels overlap the other's.  LaneSet owns their streams, events, pinned buffers and captured steps;
// DonePoll is the done-flag look generate() and generate_beam() share.  Host code, included by engine.hip only (after fail() / HIP_TRY).
#pragma once
#include "step.h"   // hold_kernel

namespace txo {

struct LaneSet {
    static constexpr int MAXL = 4;
    // captured steps, by what they were built for: built in ONE place, Session::graph_key (session.h: the range, eos, and every field of the
    // session a step's launches depend on).  Per-row stop replays a step per row count of the shrinking range (multiples of 16): a handful of
    // entries per range, built once and kept across generates.  exec = the entry the current decode replays.
    using GraphKey = std::array<int, 8>;
    struct Lane {
        int b0 = 0, nb = 0;
        hipStream_t stream = nullptr;      // lane 0 runs on the caller's stream unless the tuned pair owns it
        hipStream_t own = nullptr;         // engine-owned stream
        std::map<GraphKey, std::pair<hipGraph_t, hipGraphExec_t>> graphs;
        hipGraphExec_t exec = nullptr;
    };
    Lane lane[MAXL];
    int n = 1;
    hipStream_t cap_stream = nullptr;      // graphs are captured here, never on the caller's stream
    hipEvent_t ev_fork = nullptr, ev_join[MAXL] = {}, ev_flags[MAXL] = {}, ev_live[MAXL] = {};
    int* flags_host = nullptr;             // pinned [MAXL][Tmax]: done flags of the chunk being looked at (DonePoll)
    int* live_host = nullptr;              // pinned [MAXL]: the ranges' finished-row counts on their way to the host (per-row stop), ev_live behind them
    bool tuned = false;                    // tune() ran (once per engine)

    Lane& operator[](int i) { return lane[i]; }

    static void clear_graphs(Lane& ln) {
        for (auto& g : ln.graphs) { if (g.second.second) (void)hipGraphExecDestroy(g.second.second); if (g.second.first) (void)hipGraphDestroy(g.second.first); }
        ln.graphs.clear();
    }
    ~LaneSet() {
        for (auto& ln : lane) { clear_graphs(ln); if (ln.own) (void)hipStreamDestroy(ln.own); }
        if (cap_stream) (void)hipStreamDestroy(cap_stream);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        for (int i = 0; i < MAXL; ++i) for (hipEvent_t e : {ev_join[i], ev_flags[i], ev_live[i]}) if (e) (void)hipEventDestroy(e);
        for (int* p : {flags_host, live_host}) if (p) (void)hipHostFree(p);
    }
    int init(int tmax) {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&flags_host), sizeof(int) * MAXL * tmax, hipHostMallocDefault));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&live_host), sizeof(int) * MAXL, hipHostMallocDefault));
        for (int i = 1; i < MAXL; ++i) HIP_TRY(hipStreamCreateWithFlags(&lane[i].own, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&cap_stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
        for (int i = 0; i < MAXL; ++i)
            for (hipEvent_t* e : {&ev_join[i], &ev_flags[i], &ev_live[i]}) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
        return 0;
    }

    // Split `rows` into n contiguous ranges of whole units (16-row tiles; a beam search's ranges are whole images of `unit` beams), as even
    // as the units allow; range 0 on s, the others on the engine's streams (range 0 too once tune() picked a pair and there are two ranges).
    void split(int rows, int want, hipStream_t s, int unit = 16) {
        const int units = (rows + unit - 1) / unit;
        n = std::max(1, std::min(want, units));
        int row = 0;
        for (int i = 0; i < n; ++i) {
            lane[i].b0 = row;
            lane[i].nb = std::min(rows - row, (units / n + (i < units % n ? 1 : 0)) * unit);
            row += lane[i].nb;
            lane[i].stream = i == 0 ? s : lane[i].own;
        }
        if (n >= 2 && lane[0].own) lane[0].stream = lane[0].own;
    }
    // the ranges' streams wait for what s has enqueued so far / s waits for every range
    int fork(hipStream_t s) {
        if (n < 2) return 0;
        HIP_TRY(hipEventRecord(ev_fork, s));
        for (int i = 0; i < n; ++i) if (lane[i].stream != s) HIP_TRY(hipStreamWaitEvent(lane[i].stream, ev_fork, 0));
        return 0;
    }
    int join(hipStream_t s) {
        for (int i = 0; i < n; ++i) {
            if (lane[i].stream == s) continue;
            HIP_TRY(hipEventRecord(ev_join[i], lane[i].stream));
            HIP_TRY(hipStreamWaitEvent(s, ev_join[i], 0));
        }
        return 0;
    }
    // Error exit of a decode loop that forked: kernels of the failed call may still be running on the ranges' streams on the engine's
    // buffers.  s is made to wait for every range, drained, and the decode goes back to one range of `rows`; the error code passes through.
    int abandon(hipStream_t s, int rows, int rc) {
        for (int i = 0; i < n; ++i) {
            if (lane[i].stream == s) continue;
            if (hipEventRecord(ev_join[i], lane[i].stream) == hipSuccess) (void)hipStreamWaitEvent(s, ev_join[i], 0);
            else (void)hipStreamSynchronize(lane[i].stream);
        }
        (void)hipStreamSynchronize(s);
        (void)hipGetLastError();
        split(rows, 1, s);
        return rc;
    }

    // lane li's captured step for `key`: true = cached (it becomes the lane's exec); false = capture one and add() it
    // (shapes keep changing: at 64 entries the cache starts over rather than grow without bound)
    bool cached(int li, const GraphKey& key) {
        Lane& ln = lane[li];
        auto it = ln.graphs.find(key);
        if (it != ln.graphs.end()) { ln.exec = it->second.second; return true; }
        if (ln.graphs.size() >= 64) clear_graphs(ln);
        return false;
    }
    void add(int li, const GraphKey& key, hipGraph_t g, hipGraphExec_t e) { lane[li].graphs[key] = {g, e}; lane[li].exec = e; }

    // Two row ranges need two streams whose launches really run side by side.  Which HIP streams do depends on how the runtime mapped them onto
    // hardware queues -- on every stream the process created before (profiles/r06_b256_stream_pairs.txt: 66 / 72 / 80 / 110 ms per generate at
    // batch 256 for the same engine) -- so the pair is CHOSEN by measurement, once per engine, the first time two ranges are wanted (TXO_TUNE_LANES=0:
    // never; range 0 then stays on the caller's stream, as r02-r05): NCAND candidate streams, every pair timed on two chains of 64 launches that
    // hold one wave per CU for 4 us each behind a gate.  Pairs that share a hardware queue take twice as long (0.68 against 0.34 ms: nothing in
    // between) -- a decode on such a pair runs its ranges one after the other (110 ms per generate at batch 256 instead of 66) -- and the first
    // pair that runs side by side becomes lane[0].own / lane[1].own.  ~15 ms.  (What it does NOT remove: among pairs that do run side by side a
    // generate still takes 66-78 ms by PROCESS, whatever the pair; a trial of real decode positions per pair was built and predicts nothing.)
    int tune(int n_cus, bool verbose) {
        tuned = true;
        constexpr int NCAND = 5, CHAIN = 64;
        struct Tmp {                                                       // freed on every exit; the chosen pair is taken out
            hipStream_t cand[NCAND] = {}; hipEvent_t e0 = nullptr, ea = nullptr, eb = nullptr;
            ~Tmp() { for (auto c : cand) if (c) (void)hipStreamDestroy(c); for (auto e : {e0, ea, eb}) if (e) (void)hipEventDestroy(e); }
        } tmp;
        hipStream_t* const cand = tmp.cand;
        for (int i = 0; i < NCAND; ++i) HIP_TRY(hipStreamCreateWithFlags(&cand[i], hipStreamNonBlocking));
        HIP_TRY(hipEventCreate(&tmp.e0)); HIP_TRY(hipEventCreate(&tmp.ea)); HIP_TRY(hipEventCreate(&tmp.eb));
        auto run_pair = [&](hipStream_t a, hipStream_t b) -> double {
            double best = 1e30;
            for (int rep = 0; rep < 2; ++rep) {
                (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b);
                hipLaunchKernelGGL(hold_kernel, dim3(1), dim3(64), 0, a, 100000);          // the gate: the host enqueues both chains behind it
                (void)hipEventRecord(tmp.e0, a); (void)hipStreamWaitEvent(b, tmp.e0, 0);
                for (int i = 0; i < CHAIN; ++i) {
                    hipLaunchKernelGGL(hold_kernel, dim3(n_cus), dim3(64), 0, a, 400);
                    hipLaunchKernelGGL(hold_kernel, dim3(n_cus), dim3(64), 0, b, 400);
                }
                (void)hipEventRecord(tmp.ea, a); (void)hipEventRecord(tmp.eb, b);
                (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b);
                float ta = 0, tb = 0;
                (void)hipEventElapsedTime(&ta, tmp.e0, tmp.ea); (void)hipEventElapsedTime(&tb, tmp.e0, tmp.eb);
                best = std::min(best, (double)std::max(ta, tb));
            }
            return best;
        };
        (void)run_pair(cand[0], cand[1]);                                  // (code object load, clocks)
        double tp[NCAND][NCAND] = {}, bt = 1e30, wt = 0;
        for (int i = 0; i < NCAND; ++i)
            for (int j = i + 1; j < NCAND; ++j) { tp[i][j] = run_pair(cand[i], cand[j]); bt = std::min(bt, tp[i][j]); wt = std::max(wt, tp[i][j]); }
        int bi = 0, bj = 1; double best = 1e30;
        for (int i = 0; i < NCAND; ++i)
            for (int j = i + 1; j < NCAND; ++j) {
                if (tp[i][j] > 1.3 * bt) continue;                         // (one after the other)
                if (verbose) fprintf(stderr, "[txo] streams (%d, %d): side-by-side test %.2f ms\n", i, j, tp[i][j]);
                if (best > 1e29) { best = tp[i][j]; bi = i; bj = j; }      // the first pair that runs side by side
            }
        if (lane[0].own) (void)hipStreamDestroy(lane[0].own);
        if (lane[1].own) (void)hipStreamDestroy(lane[1].own);
        lane[0].own = cand[bi]; lane[1].own = cand[bj];
        cand[bi] = cand[bj] = nullptr;
        if (verbose) fprintf(stderr, "[txo] row-range streams: pair (%d, %d) of %d candidates (serialised pairs take %.2f ms)\n", bi, bj, NCAND, wt);
        HIP_TRY(hipGetLastError());
        return 0;
    }
};

// GLOBAL eos break (decoder.py:115-116) without draining the stream: the device records a range's done flag per position; at every CHUNK
// boundary the flags of that chunk are copied to pinned memory behind each range's steps, AHEAD more positions are enqueued, and only then
// the host waits for the copies -- the GPU keeps running those steps meanwhile (a full stream sync at every chunk left it idle for the host's
// wake-up + re-enqueue time: 1.2 ms per 256 steps).  A range's flag stays set once set, so the batch is done at the first position at which
// every range's flag is set.  After a break at most AHEAD extra positions have run; what they wrote lies beyond `steps`.
struct DonePoll {
    static constexpr int CHUNK = 32, AHEAD = 4;
    static_assert(AHEAD < CHUNK, "a chunk's flags are looked at before the next chunk's are requested");
    LaneSet& lanes; const int* done_flag; int tmax, n_pos;
    int steps = n_pos;                     // positions to return
    bool done = false;                     // every range's flag was set at position steps - 1
    int lo = -1, hi = -1;                  // chunk whose flags are in flight to the host
    // after the launches of position t; then stop enqueueing if `done`
    int after(int t) {
        const bool last = t + 1 == n_pos;
        if (lo >= 0 && (t == hi + AHEAD || last)) { if (int r = look()) return r; if (done) return 0; }
        if ((t + 1) % CHUNK == 0 || last) {
            const int c0 = (t / CHUNK) * CHUNK;
            for (int i = 0; i < lanes.n; ++i) {
                const size_t o = (size_t)i * tmax + c0;
                HIP_TRY(hipMemcpyAsync(lanes.flags_host + o, done_flag + o, sizeof(int) * (t + 1 - c0), hipMemcpyDeviceToHost, lanes[i].stream));
                HIP_TRY(hipEventRecord(lanes.ev_flags[i], lanes[i].stream));
            }
            lo = c0; hi = t;
            if (last) return look();
        }
        return 0;
    }
    int look() {                           // wait for the pending chunk's flags
        for (int i = 0; i < lanes.n; ++i) HIP_TRY(hipEventSynchronize(lanes.ev_flags[i]));
        for (int k = lo; k <= hi && !done; ++k) {
            bool all = true;
            for (int i = 0; i < lanes.n; ++i) all = all && lanes.flags_host[(size_t)i * tmax + k];
            if (all) { steps = k + 1; done = true; }
        }
        lo = -1;
        return 0;
    }
};

}  // namespace txo
