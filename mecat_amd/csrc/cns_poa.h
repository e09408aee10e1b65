// cns_poa.h — one POA window's consensus: what meap_cns_one_indel (mecat2cns/mecat_correction.cpp:62-78) computes with an AlnGraphBoost
// (mecat2cns/MECAT_AlnGraphBoost.C), restated on flat arrays, one routine for the host (libcns_poa_host.so, plain g++) and for the
// device (cns_poa.hip).  tests/test_cns_poa_ref_cpu.py holds it against the compiled reference byte for byte.
//
// The graph is adjacency_list<vecS, vecS, bidirectionalS>: every vertex has an out-list and an in-list in insertion order, add_edge
// appends to both, clear_vertex erases the vertex's edges from its neighbours' lists and keeps their order, and nothing is ever reaped
// (reapNodes is not called): a merged-away vertex stays as an isolated vertex.  Here an edge is one slot in two doubly linked lists
// (its source's out-list, its target's in-list) with head and tail per vertex: append at the tail, erase anywhere, order kept.
//
//   AlnGraphBoost(blen), blen = se - sb + 1 (:76-97)   vertices 0 .. blen + 1, 0 = '^', blen + 1 = '$', the others base 'N' weight 1;
//                  the chain i -> i + 1 with count 0; _bbMap holds the blen backbone vertices only, so a lookup of '^' or '$' default-
//                  inserts 0: both map to vertex 0.
//   addAln(q, t, start = sb_out - sb + 1) (:99-152)     double-gap columns skipped; a column with two different letters changes nothing,
//                  not even bbPos; addEdge (:199-217) increments an existing in-edge or appends a new one with count 1.
//   mergeNodes / mergeInNodes / mergeOutNodes (:219-357)   the FIFO of seed nodes, the visited flags, groups by base in std::map<char>
//                  order (ascending signed byte), members in list order, the first member survives, *anoi / *anii are the survivor's
//                  first out- / in-edge.  mergeInNodes recurses; here a frame per call on an explicit stack, its groups collected when
//                  the frame is made, as the reference's local map is.
//                  The reference adds (n1, an) for every in-edge (n1, n) of a merged-away n that has no (n1, an) yet and then clears n.
//                  Here such an edge slot MOVES: it leaves n1's out-list where it stood and n's in-list, and is appended to n1's
//                  out-list and an's in-list with its count and visited flag — the lists the reference ends up with (erase keeps
//                  order, add_edge appends; the lookups edge(n1', an) of the loop never look at an edge into n).  So no edge slot is
//                  created after the last addAln.
//   bestPath (:508-592)   float scores (small multiples of 0.5, exact); -10 for a backbone vertex of weight 1, otherwise count -
//                  coverage(_bbMap[v]) * 0.5 + score; strict >, so the first maximum in out-list order wins; nodeScore default-inserts 0;
//                  the backwards FIFO; the forward walk stops at the first vertex without a best edge.
//   consensus(minWeight, cns) (:417-458)   the longest run of path vertices with weight >= minWeight, the first one on ties;
//                  minWeight = (int)(cov * 0.4), the product in double.
//
// CAPACITIES.  With I = the insertion columns of the pieces (q a letter, t a gap) and A = the addEdge calls (match columns + insertion
// columns + one per piece):
//   nodes   blen + 2 + I        every vertex is a constructor vertex or comes from one insertion column
//   edges   blen + 1 + A        the chain, at most one new slot per addEdge call, none afterwards (moves, see above)
//   queue   nodes               mergeNodes pushes a vertex once: an edge is visited iff its source was popped (merge copies keep the
//                               source or join two unpopped vertices), so when v is pushed all its predecessors were popped, and none
//                               is popped again; bestPath pushes a vertex when its last out-edge is visited, once.  Both queues only
//                               grow from index 0, so `nodes` entries hold all pushes.
//   stack   nodes frames, nodes members in all frames together: a frame's vertex is the survivor of a group of the frame below, an
//                               ancestor in a DAG, so the frames' vertices are distinct; a member has out-degree 1, its one edge goes to
//                               its frame's vertex, and it keeps that edge while the frame lives, so the frames' member sets are disjoint.
//   output  nodes - 2           a path visits a vertex once, '^' and '$' are not written
// Both are at most blen + 2 + sum(ncols) and blen + 1 + sum(ncols + 1), the bound from the column counts alone; cns_poa_count gives I
// and A exactly.  Every capacity is checked before a write: a shortfall returns a CNS_POA_E* code and nothing is written past an array.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CNS_POA_HD __host__ __device__
#else
#define CNS_POA_HD
#endif
#if !defined(__HIP_DEVICE_COMPILE__)
#include <assert.h>
#define CNS_POA_HOST_ASSERT(x) assert(x)
#else
#define CNS_POA_HOST_ASSERT(x) ((void)0)
#endif

enum { CNS_POA_OK = 0, CNS_POA_ENODES = 1, CNS_POA_EEDGES = 2, CNS_POA_EQUEUE = 3, CNS_POA_ESTACK = 4, CNS_POA_EOUT = 5, CNS_POA_EINPUT = 6 };
enum { CNS_POA_NODE_WORDS = 17, CNS_POA_EDGE_WORDS = 8 };

// 32-bit words of workspace for these capacities
CNS_POA_HD inline long long cns_poa_words(long long nodes, long long edges) { return CNS_POA_NODE_WORDS * nodes + CNS_POA_EDGE_WORDS * edges; }

struct CnsPoaStats {
    int32_t nodes, edges, queue, frames, members;                             // high-water marks of one call
    int32_t in_merges, in_recursive, out_merges, exists, ties, stops_early;     // what happened (the tests' census): groups merged, in-groups merged
};                                                                               // below the first frame, moves that found their edge, best edges tied, a path that ends before '$'

// the insertion columns and addEdge calls of one piece (see CAPACITIES)
CNS_POA_HD inline void cns_poa_count(const char* q, const char* t, int ncols, long long* ins, long long* calls) {
    long long i = 0, a = 1;
    for (int c = 0; c < ncols; ++c) {
        const char qb = q[c], tb = t[c];
        if (qb == '-' && tb == '-') continue;
        if (qb == tb) ++a;
        else if (qb != '-' && tb == '-') { ++i; ++a; }
    }
    *ins += i; *calls += a;
}

struct CnsPoaGraph {
    int32_t ncap, ecap, nn, ne;
    int32_t *base, *weight, *cover, *bbmap, *ohead, *otail, *ihead, *itail, *odeg, *ideg, *queue, *smem, *fr_n, *fr_cur, *fr_end, *best;
    float* score;
    int32_t *src, *dst, *cnt, *vis, *onext, *oprev, *inext, *iprev;
    CnsPoaStats st;

    CNS_POA_HD void carve(int32_t* w, int32_t nodes, int32_t edges) {
        ncap = nodes; ecap = edges; nn = ne = 0;
        int32_t** na[] = {&base, &weight, &cover, &bbmap, &ohead, &otail, &ihead, &itail, &odeg, &ideg, &queue, &smem, &fr_n, &fr_cur, &fr_end, &best};
        for (int k = 0; k < 16; ++k) { *na[k] = w; w += nodes; }
        score = reinterpret_cast<float*>(w); w += nodes;
        int32_t** ea[] = {&src, &dst, &cnt, &vis, &onext, &oprev, &inext, &iprev};
        for (int k = 0; k < 8; ++k) { *ea[k] = w; w += edges; }
        st = CnsPoaStats();
    }
    CNS_POA_HD int add_vertex(int b, int wt, int bb) {
        if (nn >= ncap) return -1;
        const int v = nn++;
        base[v] = b; weight[v] = wt; cover[v] = 0; bbmap[v] = bb;
        ohead[v] = otail[v] = ihead[v] = itail[v] = -1; odeg[v] = ideg[v] = 0;
        return v;
    }
    CNS_POA_HD void link(int e, int u, int v) {          // add_edge's two push_backs
        src[e] = u; dst[e] = v;
        onext[e] = -1; oprev[e] = otail[u];
        if (otail[u] < 0) ohead[u] = e; else onext[otail[u]] = e;
        otail[u] = e; ++odeg[u];
        inext[e] = -1; iprev[e] = itail[v];
        if (itail[v] < 0) ihead[v] = e; else inext[itail[v]] = e;
        itail[v] = e; ++ideg[v];
    }
    CNS_POA_HD void unlink_out(int e) {
        const int u = src[e];
        if (oprev[e] < 0) ohead[u] = onext[e]; else onext[oprev[e]] = onext[e];
        if (onext[e] < 0) otail[u] = oprev[e]; else oprev[onext[e]] = oprev[e];
        --odeg[u];
    }
    CNS_POA_HD void unlink_in(int e) {
        const int v = dst[e];
        if (iprev[e] < 0) ihead[v] = inext[e]; else inext[iprev[e]] = inext[e];
        if (inext[e] < 0) itail[v] = iprev[e]; else iprev[inext[e]] = iprev[e];
        --ideg[v];
    }
    CNS_POA_HD int new_edge(int u, int v, int count) {
        if (ne >= ecap) return -1;
        const int e = ne++;
        cnt[e] = count; vis[e] = 0;
        link(e, u, v);
        return e;
    }
    CNS_POA_HD int add_edge_counted(int u, int v) {     // addEdge (:199-217); 0 or CNS_POA_EEDGES
        bool exists = false;
        for (int e = ihead[v]; e >= 0; e = inext[e])
            if (src[e] == u) { ++cnt[e]; exists = true; }
        if (!exists && new_edge(u, v, 1) < 0) return CNS_POA_EEDGES;
        return 0;
    }
    CNS_POA_HD int find_edge(int u, int v) const {      // edge(u, v, g): the first one in u's out-list
        for (int e = ohead[u]; e >= 0; e = onext[e])
            if (dst[e] == v) return e;
        return -1;
    }
    CNS_POA_HD void clear_vertex(int v) {
        for (int e = ohead[v]; e >= 0; e = onext[e]) unlink_in(e);
        for (int e = ihead[v]; e >= 0; e = inext[e]) unlink_out(e);
        ohead[v] = otail[v] = ihead[v] = itail[v] = -1; odeg[v] = ideg[v] = 0;
    }
    // smem[m0, return): the vertices a merge groups — sources of n's in-edges with out-degree 1 (IN) or targets of its out-edges with
    // in-degree 1 — in std::map<char, vector> order: ascending base as a signed char, list order inside a base (a stable insertion sort).
    // -1: no room
    template <bool IN>
    CNS_POA_HD int collect(int n, int m0) {
        int m1 = m0;
        for (int e = IN ? ihead[n] : ohead[n]; e >= 0; e = IN ? inext[e] : onext[e]) {
            const int x = IN ? src[e] : dst[e];
            if ((IN ? odeg[x] : ideg[x]) != 1) continue;
            if (m1 >= ncap) return -1;
            int k = m1++;
            const int bx = (signed char)base[x];
            while (k > m0 && (signed char)base[smem[k - 1]] > bx) { smem[k] = smem[k - 1]; --k; }
            smem[k] = x;
        }
        if (m1 > st.members) st.members = m1;
        return m1;
    }
    // one group smem[g0, g1) of mergeInNodes (:269-302) / mergeOutNodes (:322-355); -1 when a list that must have an edge has none
    template <bool IN>
    CNS_POA_HD int merge_group(int g0, int g1) {
        const int an = smem[g0];
        const int ane = IN ? ohead[an] : ihead[an];
        if (ane < 0) return -1;
        for (int k = g0 + 1; k < g1; ++k) {
            const int x = smem[k];
            const int xe = IN ? ohead[x] : ihead[x];
            if (xe < 0) return -1;
            cnt[ane] += cnt[xe];
            weight[an] += weight[x];
        }
        for (int k = g0 + 1; k < g1; ++k) {
            const int x = smem[k];
            for (int e = IN ? ihead[x] : ohead[x], nx; e >= 0; e = nx) {
                nx = IN ? inext[e] : onext[e];
                const int y = IN ? src[e] : dst[e];
                const int f = IN ? find_edge(y, an) : find_edge(an, y);
                if (f >= 0) { cnt[f] += cnt[e]; ++st.exists; }
                else {                      // the edge moves (see the header comment): count and visited stay with it
                    unlink_out(e); unlink_in(e);
                    if (IN) link(e, y, an); else link(e, an, y);
                }
            }
            clear_vertex(x);                // markForReaper (:359-363)
        }
        return an;
    }
    CNS_POA_HD int merge_in(int n0) {       // mergeInNodes (:252-305), its recursion as frames
        int depth = 0;
        int m = collect<true>(n0, 0);
        if (m < 0) return CNS_POA_ESTACK;
        fr_n[0] = n0; fr_cur[0] = 0; fr_end[0] = m; depth = 1;
        if (st.frames < 1) st.frames = 1;
        while (depth > 0) {
            const int f = depth - 1;
            const int g0 = fr_cur[f];
            if (g0 >= fr_end[f]) { --depth; continue; }
            int g1 = g0 + 1;
            while (g1 < fr_end[f] && base[smem[g1]] == base[smem[g0]]) ++g1;
            fr_cur[f] = g1;
            if (g1 - g0 <= 1) continue;
            const int an = merge_group<true>(g0, g1);
            if (an < 0) return CNS_POA_EINPUT;
            ++st.in_merges; st.in_recursive += depth > 1;
            if (depth >= ncap) return CNS_POA_ESTACK;
            m = collect<true>(an, fr_end[f]);
            if (m < 0) return CNS_POA_ESTACK;
            fr_n[depth] = an; fr_cur[depth] = fr_end[f]; fr_end[depth] = m; ++depth;
            if (depth > st.frames) st.frames = depth;
        }
        return 0;
    }
    CNS_POA_HD int merge_out(int n) {       // mergeOutNodes (:307-357)
        const int m = collect<false>(n, 0);
        if (m < 0) return CNS_POA_ESTACK;
        for (int g0 = 0, g1; g0 < m; g0 = g1) {
            g1 = g0 + 1;
            while (g1 < m && base[smem[g1]] == base[smem[g0]]) ++g1;
            if (g1 - g0 <= 1) continue;
            if (merge_group<false>(g0, g1) < 0) return CNS_POA_EINPUT;
            ++st.out_merges;
        }
        return 0;
    }
    CNS_POA_HD int merge_nodes() {          // mergeNodes (:219-250)
        int head = 0, tail = 0;
        queue[tail++] = 0;
        while (head < tail) {
            const int u = queue[head++];
            int rc = merge_in(u);
            if (rc) return rc;
            rc = merge_out(u);
            if (rc) return rc;
            for (int e = ohead[u]; e >= 0; e = onext[e]) {
                vis[e] = 1;
                const int v = dst[e];
                int not_visited = 0;
                for (int i = ihead[v]; i >= 0; i = inext[i]) not_visited += !vis[i];
                if (not_visited == 0) {
                    if (tail >= ncap) return CNS_POA_EQUEUE;
                    queue[tail++] = v;
                }
            }
        }
        if (tail > st.queue) st.queue = tail;
        return 0;
    }
    CNS_POA_HD int best_path(int blen) {    // bestPath (:508-573), up to the forward walk
        for (int e = 0; e < ne; ++e) vis[e] = 0;
        for (int v = 0; v < nn; ++v) { score[v] = 0.0f; best[v] = -1; }
        int head = 0, tail = 0;
        queue[tail++] = blen + 1;
        while (head < tail) {
            const int n = queue[head++];
            bool found = false, tie = false;
            float best_score = -3.402823466e+38f;
            int best_edge = -1;
            for (int e = ohead[n]; e >= 0; e = onext[e]) {
                const int o = dst[e];
                const float s = score[o];
                float ns;
                if (o <= blen + 1 && weight[o] == 1) ns = s - 10.0f;
                else ns = (float)cnt[e] - (float)cover[bbmap[o]] * 0.5f + s;
                if (ns > best_score) { best_score = ns; best_edge = e; found = true; tie = false; }
                else if (ns == best_score) tie = true;
            }
            if (found) { score[n] = best_score; best[n] = best_edge; st.ties += tie; }
            for (int i = ihead[n]; i >= 0; i = inext[i]) {
                vis[i] = 1;
                const int p = src[i];
                int not_visited = 0;
                for (int e = ohead[p]; e >= 0; e = onext[e]) not_visited += !vis[e];
                if (not_visited == 0) {
                    if (tail >= ncap) return CNS_POA_EQUEUE;
                    queue[tail++] = p;
                }
            }
        }
        if (tail > st.queue) st.queue = tail;
        return 0;
    }
};

// (int)(cov * 0.4) as the call ag.consensus(min_cov * 0.4, cns) converts it (mecat_correction.cpp:77)
CNS_POA_HD inline int cns_poa_min_weight(int cov) { return (int)((double)cov * 0.4); }

// One window.  get(k, &q, &t, &ncols, &sb_out) hands out piece k of npieces in add order: q / t point at the piece's first column of
// qaln / saln.  w: cns_poa_words(nodes, edges) words of workspace.  out[out_cap] takes the string ag.consensus(cov * 0.4, cns) returns,
// *out_len its length (0 on error).  -> CNS_POA_OK or the capacity that would have been exceeded; CNS_POA_EINPUT for a piece that leaves
// the backbone (the reference indexes past its vertices there).  stats may be NULL.
template <class Get>
CNS_POA_HD inline int cns_poa_window(int sb, int se, int cov, const Get& get, int npieces, int32_t* w, int32_t nodes, int32_t edges, char* out, int32_t out_cap,
                                     int32_t* out_len, CnsPoaStats* stats) {
    *out_len = 0;
    const long long blen64 = (long long)se - sb + 1;
    if (blen64 < 1 || blen64 + 2 > nodes) return blen64 < 1 ? CNS_POA_EINPUT : CNS_POA_ENODES;
    if (blen64 + 1 > edges) return CNS_POA_EEDGES;
    const int blen = (int)blen64;
    CnsPoaGraph g;
    g.carve(w, nodes, edges);
    g.add_vertex('^', 0, 0);
    for (int i = 1; i <= blen; ++i) g.add_vertex('N', 1, i);
    g.add_vertex('$', 0, 0);
    for (int i = 0; i <= blen; ++i) g.new_edge(i, i + 1, 0);
    int rc = 0;
    for (int k = 0; k < npieces && !rc; ++k) {       // addAln (:99-152)
        const char *q, *t;
        int ncols, sb_out;
        get(k, &q, &t, &ncols, &sb_out);
        long long bb = (long long)sb_out - sb + 1;
        int prev = 0;
        for (int c = 0; c < ncols && !rc; ++c) {
            const char qb = q[c], tb = t[c];
            if (qb == '-' && tb == '-') continue;
            if (qb == tb || qb == '-') {
                if (bb < 0 || bb > blen + 1) { rc = CNS_POA_EINPUT; break; }
                const int cur = (int)bb;
                ++g.cover[g.bbmap[cur]];
                g.base[g.bbmap[cur]] = tb;
                if (qb == tb) {
                    ++g.weight[cur];
                    rc = g.add_edge_counted(prev, cur);
                    prev = cur;
                }
                ++bb;
            } else if (tb == '-') {
                if (bb < 0 || bb > blen + 1) { rc = CNS_POA_EINPUT; break; }
                const int v = g.add_vertex(qb, 1, (int)bb);
                if (v < 0) { rc = CNS_POA_ENODES; break; }
                rc = g.add_edge_counted(prev, v);
                prev = v;
            }
        }
        if (!rc) rc = g.add_edge_counted(prev, blen + 1);
    }
    g.st.nodes = g.nn; g.st.edges = g.ne;
    if (!rc) rc = g.merge_nodes();
    if (!rc) rc = g.best_path(blen);
    if (rc) { if (stats) *stats = g.st; return rc; }
    // consensus (:417-458): the path is walked twice, for the run and for its letters
    const int min_weight = cns_poa_min_weight(cov);
    int offs = 0, best_offs = 0, length = 0, idx = 0;
    bool met = false;
    for (int v = 0, steps = 0;; ++steps) {
        if (steps > g.nn) return CNS_POA_EINPUT;      // (a path visits a vertex once)
        if (g.base[v] != '^' && g.base[v] != '$') {
            if (!met && g.weight[v] >= min_weight) { offs = idx; met = true; }
            else if (met && g.weight[v] < min_weight) {
                if (idx - offs > length) { best_offs = offs; length = idx - offs; }
                met = false;
            }
            ++idx;
        }
        if (g.best[v] < 0) { g.st.stops_early = v != blen + 1; break; }
        v = g.dst[g.best[v]];
    }
    if (stats) *stats = g.st;
    if (met && idx - offs > length) { best_offs = offs; length = idx - offs; }
    CNS_POA_HOST_ASSERT(idx <= g.nn - 2 || g.nn < 2);
    if (length > out_cap) return CNS_POA_EOUT;
    idx = 0;
    for (int v = 0;;) {
        if (g.base[v] != '^' && g.base[v] != '$') {
            if (idx >= best_offs && idx < best_offs + length) out[idx - best_offs] = (char)g.base[v];
            ++idx;
        }
        if (g.best[v] < 0 || idx >= best_offs + length) break;
        v = g.dst[g.best[v]];
    }
    *out_len = length;
    return CNS_POA_OK;
}
