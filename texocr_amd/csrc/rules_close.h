// Closing decode (texocr.h: txo_set_rules_close): how far every node of a rule set's automaton is from a committed eos.  Plain C++, no
// device code and no HIP header: the engine calls it at installation, and a stand-alone host program can call it as well.
//
// A node is (s, d): state s < S at depth 0 <= d <= depth_max.  dist[s][d] is the least number of picks, the eos included, that takes a row
// from (s, d) to a committed eos when every pick on the way is one the rule allows (step_rules.h: rule_allows) and every move is the rule's
// own (next, clamp(d + delta, 0, depth_max)); CLOSE_INF: no such path.  So dist == 1 exactly where eos itself is allowed.
//
// A state's row is first reduced to its distinct (need, delta, next, flags) words -- a byte-level vocabulary has a handful of them among its
// thousand tokens -- so the search walks a few edges per node, not V.  The search itself is a breadth-first search from the eos over the
// reversed edges: at most 8 * 256 nodes, unit edge weights.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace txo {

constexpr int32_t CLOSE_INF = 0x7fffffff;

namespace close_detail {
// the fields of a packed entry (the layout of step_rules.h / texocr.h, restated so that this header stands without them)
constexpr int32_t BAN = 1 << 24, ONLY_AT_ZERO = 1 << 25, FIELDS = (1 << 26) - 1;
inline int need(int32_t r) { return r & 0xff; }
inline int delta(int32_t r) { return (int)(signed char)((r >> 8) & 0xff); }
inline int next(int32_t r) { return (r >> 16) & 0xff; }
inline bool allows(int32_t r, int d, int depth_max) {
    return !(r & BAN) && d >= need(r) && d + delta(r) <= depth_max && (!(r & ONLY_AT_ZERO) || d == 0);
}
inline int depth_after(int32_t r, int d, int depth_max) { return std::min(std::max(d + delta(r), 0), depth_max); }
}  // namespace close_detail

// rules [S][V] packed entries, 1 <= S, 1 <= depth_max, every next < S (txo_set_token_rules has checked all three); eos outside [0, V): no
// node reaches it.  dist_out: [S][depth_max + 1], resized here.  Returns dist_max, the largest finite entry (0: every entry is CLOSE_INF);
// *any_inf (may be null): some entry is CLOSE_INF.
inline int rules_close_dist(const int32_t* rules, int S, int V, int depth_max, int eos, std::vector<int32_t>& dist_out, bool* any_inf = nullptr) {
    using namespace close_detail;
    const int W = depth_max + 1, N = S * W;
    dist_out.assign((size_t)N, CLOSE_INF);
    if (any_inf) *any_inf = N > 0;
    if (eos < 0 || eos >= V || N <= 0) return 0;
    // the distinct words of every state's non-eos tokens that can ever be picked
    std::vector<std::vector<int32_t>> words((size_t)S);
    for (int s = 0; s < S; ++s) {
        std::vector<int32_t>& w = words[(size_t)s];
        w.reserve((size_t)V);
        for (int v = 0; v < V; ++v) {
            const int32_t r = rules[(size_t)s * V + v] & FIELDS;
            if (v != eos && !(r & BAN) && next(r) < S) w.push_back(r);
        }
        std::sort(w.begin(), w.end());
        w.erase(std::unique(w.begin(), w.end()), w.end());
    }
    // reversed edges: pred[n] = the nodes with an allowed non-eos move into n (a node may be listed twice: harmless)
    std::vector<std::vector<int32_t>> pred((size_t)N);
    std::vector<int32_t> frontier, nxt;
    for (int s = 0; s < S; ++s)
        for (int d = 0; d < W; ++d) {
            const int n = s * W + d;
            for (const int32_t r : words[(size_t)s])
                if (allows(r, d, depth_max)) pred[(size_t)(next(r) * W + depth_after(r, d, depth_max))].push_back(n);
            if (allows(rules[(size_t)s * V + eos], d, depth_max)) { dist_out[(size_t)n] = 1; frontier.push_back(n); }
        }
    int dist_max = frontier.empty() ? 0 : 1;
    for (int level = 2; !frontier.empty(); ++level) {
        nxt.clear();
        for (const int32_t n : frontier)
            for (const int32_t p : pred[(size_t)n])
                if (dist_out[(size_t)p] == CLOSE_INF) { dist_out[(size_t)p] = level; nxt.push_back(p); dist_max = level; }
        frontier.swap(nxt);
    }
    if (any_inf) *any_inf = std::find(dist_out.begin(), dist_out.end(), CLOSE_INF) != dist_out.end();
    return dist_max;
}

}  // namespace txo
