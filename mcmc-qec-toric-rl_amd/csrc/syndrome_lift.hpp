// From bare syndromes to start chains: the LIFT TABLE of a code -- one packed Pauli string per check whose syndrome is that check alone (on the
// torus: plus the root check of its component) -- and the lift-and-descend body that turns a defect array into a chain with that syndrome.
// No matching: chain = XOR of the table rows of the set cells, then (optionally) a greedy descent over the stabilizer generators in table order,
// a generator being applied iff it lowers the error count, whole sweeps repeated until one applies nothing (at most nq applications: nq + 1 sweeps).
// The result is a local minimum of the weight, in an arbitrary equivalence class.
//
// The table builder is pure host C++ (like tables.hpp).  lift_body() is ONE __host__ __device__ function: syndrome_lift.hip runs it with one lane per
// syndrome and the state in LDS, tables_test_api.cpp and syndrome_lift_selftest.cpp run it by g++ on a plain array -- the tests compare the two bit for bit.
#pragma once
#include "../../include/qecmc.h"

#include <cstdint>
#include <vector>

#include "stencil_bytes.hpp"   // code_nq_of / surf_ngen: the codes' dimensions
#include "tables.hpp"          // toric_generator_table / surf_generator_table

namespace qecmc {
namespace lift {

// cells of the defect layout qecmc_syndrome writes: toric uint8[2][L][L]; xzzx / rotated uint8[L+1][L+1] (only some are checks);
// planar vertex defects [L-1][L] then plaquette defects [L][L-1]
inline int defect_cells(int code, int L)
{
    return code == QECMC_TORIC ? 2 * L * L : code == QECMC_PLANAR ? 2 * L * (L - 1) : (L + 1) * (L + 1);
}

// generator g (table order) -> the defect cell its violation sets: what toric_syndrome_b / surf_syndrome_b / planar_syndrome_b (stencil_bytes.hpp) imply.
// toric: defects[0][r][c] tests the Z / Y parts of the X-type generator (r, c)'s sites, defects[1][r][c] the Z-type one's -- cell g; planar: the
// vertex defects are the X-type generators row-major, the plaquette defects the Z-type ones -- cell g; xzzx / rotated: plaquette (i, j) sits at
// (i + 1, j + 1) of the (L+1)^2 grid, half plaquette i of side 0 .. 3 on the grid's top / right / bottom / left edge
inline int generator_cell(int code, int L, int g)
{
    if (code == QECMC_TORIC || code == QECMC_PLANAR) return g;
    const int S = L + 1, nf = (L - 1) * (L - 1);
    if (g < nf) return (g / (L - 1) + 1) * S + g % (L - 1) + 1;
    const int i = (g - nf) >> 2;
    switch ((g - nf) & 3) {
        case 0: return 2 * i + 2;
        case 1: return (2 * i + 2) * S + L;
        case 2: return L * S + 2 * i + 1;
        default: return (2 * i + 1) * S;
    }
}

// The table of one (code, L).  rows: [n_cells][W + 1] -- W state words in the kernels' 2-bit packing (qubit q in word q >> 4 at bit 2 (q & 15)), then a
// FLAG word: 0 = the cell is no check (no row); else bit 0 set and, for a check of boundary-less component k (the torus), bit 1 + k -- the XOR of the
// flags of a syndrome's set cells has a bit above 0 set iff such a component holds an odd number of defects.  gen: the generator table, 2 words each.
struct Table {
    int code = 0, L = 0, nq = 0, W = 0, n_cells = 0, n_gen = 0;
    std::vector<uint32_t> rows, gen;
};

// Nodes: the check cells and one virtual boundary node.  Edges: for every qubit q ascending and P = X then Z, the cells the syndrome of P on q sets
// (the generators that act on q with another non-identity Pauli, ascending) -- none: an idle cell of the planar layout, skipped; one: an edge to the
// boundary node; two: an edge between them.  Breadth-first over adjacency lists in insertion order, from the boundary node if it has edges, then from
// every unreached check in ascending cell index (the root of its component); row(node) = row(BFS parent) XOR P on q.  Empty table: a single-qubit
// Pauli sets more than two cells, or a 32nd boundary-less component (none of the four code models does either).
inline Table build_table(int code, int L)
{
    Table t;
    t.code = code; t.L = L; t.nq = code_nq_of(code, L); t.W = (t.nq + 15) / 16; t.n_cells = defect_cells(code, L);
    t.gen = code == QECMC_TORIC ? tables::toric_generator_table(L) : tables::surf_generator_table(code, L);
    t.n_gen = (int)(t.gen.size() / 2);
    const int boundary = t.n_cells;
    struct Edge { int to, q; uint32_t pauli; };
    std::vector<std::vector<Edge>> adj((size_t)t.n_cells + 1);
    std::vector<char> is_check((size_t)t.n_cells, 0);
    // the generators on every qubit, ascending in g
    struct On { int cell; uint32_t pauli; };
    std::vector<std::vector<On>> on((size_t)t.nq);
    for (int g = 0; g < t.n_gen; ++g) {
        const int cell = generator_cell(code, L, g);
        is_check[(size_t)cell] = 1;
        for (int u = 0; u < 4; ++u) {
            const uint32_t e = (u < 2 ? t.gen[2 * (size_t)g] >> (16 * u) : t.gen[2 * (size_t)g + 1] >> (16 * (u - 2))) & 0xFFFFu;
            if (e & 3u) on[e >> 2].push_back({cell, e & 3u});
        }
    }
    for (int q = 0; q < t.nq; ++q)
        for (uint32_t P : {1u, 3u}) {
            int cells[2], n = 0;
            for (const On &o : on[(size_t)q]) {
                if (o.pauli == P) continue;          // the same Pauli commutes
                if (n == 2) return Table();
                cells[n++] = o.cell;
            }
            if (n == 0) continue;
            const int a = cells[0], b = n == 2 ? cells[1] : boundary;
            adj[(size_t)a].push_back({b, q, P});
            adj[(size_t)b].push_back({a, q, P});
        }
    const size_t stride = (size_t)t.W + 1;
    t.rows.assign((size_t)t.n_cells * stride, 0u);
    std::vector<char> seen((size_t)t.n_cells + 1, 0);
    std::vector<int> queue;
    auto bfs = [&](int start, uint32_t flag) {
        queue.assign(1, start);
        seen[(size_t)start] = 1;
        if (start != boundary) t.rows[(size_t)start * stride + t.W] = flag;
        for (size_t head = 0; head < queue.size(); ++head) {
            const int node = queue[head];
            for (const Edge &e : adj[(size_t)node]) {
                if (seen[(size_t)e.to]) continue;
                seen[(size_t)e.to] = 1;
                uint32_t *row = &t.rows[(size_t)e.to * stride];
                if (node != boundary)
                    for (int w = 0; w < t.W; ++w) row[w] = t.rows[(size_t)node * stride + w];
                row[e.q >> 4] ^= e.pauli << ((e.q & 15) * 2);
                row[t.W] = flag;
                queue.push_back(e.to);
            }
        }
    };
    if (!adj[(size_t)boundary].empty()) bfs(boundary, 1u);
    int closed = 0;
    for (int cell = 0; cell < t.n_cells; ++cell) {
        if (!is_check[(size_t)cell] || seen[(size_t)cell]) continue;
        if (closed == 31) return Table();
        bfs(cell, 1u | (2u << closed));
        ++closed;
    }
    return t;
}

__host__ __device__ inline int count_fields(uint32_t v)
{
    const uint32_t m = (v | (v >> 1)) & 0x55555555u;
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(m);
#else
    return __builtin_popcount(m);
#endif
}

// The greedy descent of lift_body() (and of correct_body(), corrections.hpp) on the state st holds: generators in table order, one applied iff it lowers
// the error count, whole sweeps until one applies nothing.  Every application lowers the count by >= 1: at most nq of them, nq + 1 sweeps.
template <class St>
__host__ __device__ inline void greedy_descent(St &st, const uint32_t *__restrict__ gen, int nq, int n_gen)
{
    for (int sweep = 0; sweep <= nq; ++sweep) {
        bool changed = false;
        for (int g = 0; g < n_gen; ++g) {
            const uint32_t e01 = gen[2 * (size_t)g], e23 = gen[2 * (size_t)g + 1];
            int dE = 0;
            for (int u = 0; u < 4; ++u) {
                const uint32_t e = (u < 2 ? e01 >> (16 * u) : e23 >> (16 * (u - 2))) & 0xFFFFu, P = e & 3u, q = e >> 2;
                if (P == 0u) continue;
                const uint32_t f = (st.get((int)(q >> 4)) >> ((q & 15u) * 2u)) & 3u;
                dE += f == 0u ? 1 : f == P ? -1 : 0;
            }
            const bool apply = dE < 0;
            for (int u = 0; u < 4; ++u) {
                const uint32_t e = (u < 2 ? e01 >> (16 * u) : e23 >> (16 * (u - 2))) & 0xFFFFu, P = e & 3u, q = e >> 2;
                if (P == 0u) continue;
                if (apply) st.set((int)(q >> 4), st.get((int)(q >> 4)) ^ (P << ((q & 15u) * 2u)));
            }
            changed |= apply;
        }
        if (!st.any(changed)) break;
    }
}

// One syndrome.  St holds W state words: get(w), set(w, v), and any(b) -- true iff b holds for some syndrome that walks the loops together with this
// one (the 64 lanes of a wavefront on the device; on the host, this one alone: a syndrome whose sweep applied nothing is at a fixed point, so the
// extra sweeps a wavefront makes for its neighbours change nothing).  Every table address depends on the loop counters only.
// defects: this syndrome's n_cells bytes, or nullptr for an idle lane.  status 0: lifted; 1: not a syndrome of this code (a set cell that is no
// check, or an odd number of defects in a boundary-less component) -- the state is then all zero and weight -1.
template <class St>
__host__ __device__ inline void lift_body(St &st, const uint32_t *__restrict__ rows, const uint32_t *__restrict__ gen, int n_cells, int W, int nq, int n_gen,
                                          const uint8_t *__restrict__ defects, int descend, int &status, int &weight)
{
    for (int w = 0; w < W; ++w) st.set(w, 0u);
    uint32_t parity = 0;
    bool stray = false;
    for (int cell = 0; cell < n_cells; ++cell) {
        const uint32_t *row = rows + (size_t)cell * (size_t)(W + 1);
        const uint32_t flag = row[W];
        const bool on = defects != nullptr && defects[cell] != 0;
        if (on) { parity ^= flag; stray |= flag == 0u; }
        if (flag == 0u) continue;
        for (int w = 0; w < W; ++w) {
            const uint32_t r = row[w];
            if (r == 0u) continue;                                   // (the same for every syndrome: most words of a row are empty)
            if (on) st.set(w, st.get(w) ^ r);
        }
    }
    status = (stray || (parity >> 1) != 0u) ? 1 : 0;
    if (status)
        for (int w = 0; w < W; ++w) st.set(w, 0u);
    if (descend) greedy_descent(st, gen, nq, n_gen);
    weight = 0;
    for (int w = 0; w < W; ++w) weight += count_fields(st.get(w));
    if (status) weight = -1;
}

// the host's state: W words in a plain array
struct HostState {
    uint32_t *words;
    uint32_t get(int w) const { return words[w]; }
    void set(int w, uint32_t v) { words[w] = v; }
    bool any(bool b) const { return b; }
};

// N syndromes on the host, one after the other: defects uint8[N][n_cells] -> chains uint8[N][nq], status uint8[N] (nullable), weight int32[N] (nullable)
inline void chains_from_syndromes_host(const Table &t, uint64_t N, const uint8_t *defects, int descend, uint8_t *chains, uint8_t *status, int32_t *weight)
{
    std::vector<uint32_t> words((size_t)t.W);
    HostState st{words.data()};
    for (uint64_t s = 0; s < N; ++s) {
        int stat = 0, wgt = 0;
        lift_body(st, t.rows.data(), t.gen.data(), t.n_cells, t.W, t.nq, t.n_gen, defects + s * (uint64_t)t.n_cells, descend, stat, wgt);
        for (int q = 0; q < t.nq; ++q) chains[s * (uint64_t)t.nq + q] = (uint8_t)((words[(size_t)(q >> 4)] >> ((q & 15) * 2)) & 3u);
        if (status) status[s] = (uint8_t)stat;
        if (weight) weight[s] = wgt;
    }
}

}  // namespace lift

// the dynamic LDS of the largest lattice check_code_L accepts (toric / planar L = 64: W = 512 words of 64 lanes): what k_syndrome_lift and
// k_corrections ask the runtime for, once per device, when a launch needs more than the default 64 KiB window
constexpr size_t kServiceLdsMax = 512u * 64u * sizeof(uint32_t);

// syndrome_lift.hip: all pointers are device pointers; status / weight nullable.  One lane per syndrome, 64-lane workgroups, W * 256 bytes of LDS.
struct LiftArgs {
    uint64_t N;
    int n_cells, W, nq, n_gen, descend;
};
hipError_t launch_syndrome_lift(const LiftArgs &a, const uint32_t *rows, const uint32_t *gen, const uint8_t *defects, uint8_t *chains, uint8_t *status,
                                int32_t *weight, hipStream_t stream);

}  // namespace qecmc
