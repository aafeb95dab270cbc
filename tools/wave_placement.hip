// Diagnostic (not part of the product): where the waves of a scan = wave workgroup are placed.  A stand-alone kernel with the headline launch's
// footprint -- 1 024 workgroups, `__launch_bounds__(512, 8)`, the dynamic LDS of toric L = 9 at the ladder's length (wu_plan_lds_bytes) -- in which every
// wave records HW_ID, XCC_ID and the clock at entry and exit around a bounded dependent-add loop (no waiting on other workgroups, no spin on memory),
// for 5, 6, 7, 8 and 9 waves per workgroup (9: the 1 024-thread bound at 4 waves per SIMD, as choose_wave gives a ladder of 9 rungs).
// ASSUMPTION: the tool's workgroups are placed as ladder_wu_kernel's are because the two have the same footprint (threads, launch bound, LDS, grid);
// nothing here measures the real kernel.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o wave_placement tools/wave_placement.hip && ./wave_placement profiles/r11_wave_placement.json
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>
#include "../mcmc-qec-toric-rl_amd/csrc/kernel_choice.hpp"
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

using namespace qecmc;

struct Stamp { uint32_t hw, xcc; uint64_t t0, t1, r0, r1; };   // t: s_memtime (a clock per shader engine), r: s_memrealtime (one for the chip)

template <int MAXT, int MINW>
__global__ __launch_bounds__(MAXT, MINW) void placement_kernel(Stamp *out, uint32_t *sink, int spins, uint32_t seed)
{
    extern __shared__ uint32_t lds[];
    const uint64_t t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    const uint32_t hw = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));    // HW_ID
    const uint32_t xcc = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11));  // XCC_ID
    uint32_t x = threadIdx.x + seed;
    for (int i = 0; i < spins; ++i) {   // bounded: `spins` dependent additions, nothing else
        x += seed;
        asm volatile("" : "+v"(x));
    }
    if (threadIdx.x == 0) lds[0] = x;   // (the LDS segment is used)
    __syncthreads();
    const uint64_t t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    const uint32_t nw = blockDim.x >> 6, wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) out[blockIdx.x * nw + wave] = Stamp{hw, xcc, t0, t1, r0, r1};   // (an ordinary per-lane store)
    if (x + lds[0] == 0x12345u) sink[0] = x;
}

static const int kGrid = 1024;
static const int kSeq[4] = {0, 2, 1, 3};   // the cyclic order in which a workgroup's waves go to SIMDs
static int seq_pos(int simd) { for (int i = 0; i < 4; ++i) if (kSeq[i] == simd) return i; return -1; }

int run(int waves, int spins, FILE *f, bool last)
{
    const int Nc = waves, W = 11, ncls = 16, L = 9;   // toric L = 9: 162 qubits in 11 words, 16 classes
    const size_t lds = wu_plan_lds_bytes(Nc, W, ncls, L, false, false, 10);
    Stamp *d; uint32_t *sink;
    CHECK(hipMalloc(&d, sizeof(Stamp) * kGrid * waves)); CHECK(hipMalloc(&sink, 4));
    CHECK(hipMemset(d, 0, sizeof(Stamp) * kGrid * waves));
    for (int rep = 0; rep < 2; ++rep) {   // (the second launch is the one recorded: code and page tables warm)
        if (waves <= 8) hipLaunchKernelGGL((placement_kernel<512, 8>), dim3(kGrid), dim3(waves * 64), lds, 0, d, sink, spins, 1u);
        else hipLaunchKernelGGL((placement_kernel<1024, 4>), dim3(kGrid), dim3(waves * 64), lds, 0, d, sink, spins, 1u);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
    }
    std::vector<Stamp> h((size_t)kGrid * waves);
    CHECK(hipMemcpy(h.data(), d, sizeof(Stamp) * h.size(), hipMemcpyDeviceToHost));
    CHECK(hipFree(d)); CHECK(hipFree(sink));

    // co-residency of the grid: the latest entry against the earliest exit on the chip's real-time clock (s_memtime differs between parts of the chip:
    // its stamps compare within a CU only, below)
    uint64_t first_in = ~0ull, last_in = 0, first_out = ~0ull, last_out = 0;
    for (const Stamp &s : h) { first_in = std::min(first_in, s.r0); last_in = std::max(last_in, s.r0); first_out = std::min(first_out, s.r1); last_out = std::max(last_out, s.r1); }
    const bool resident = last_in < first_out;

    std::map<uint32_t, std::vector<int>> percu;   // (xcc, se, sh, cu) -> workgroups
    long pair_same = 0, pair_all = 0, order_ok = 0, order_all = 0, split = 0;
    for (int b = 0; b < kGrid; ++b) {
        const Stamp &s0 = h[(size_t)b * waves];
        const uint32_t key0 = ((s0.xcc & 0xFu) << 16) | (s0.hw & 0xFF00u);
        percu[key0].push_back(b);
        for (int w = 0; w < waves; ++w) {
            const Stamp &s = h[(size_t)b * waves + w];
            if ((((s.xcc & 0xFu) << 16) | (s.hw & 0xFF00u)) != key0) ++split;
            const int simd = (s.hw >> 4) & 3;
            if (w + 4 < waves) { ++pair_all; pair_same += simd == (int)((h[(size_t)b * waves + w + 4].hw >> 4) & 3); }
            if (w + 1 < waves) { ++order_all; order_ok += seq_pos((h[(size_t)b * waves + w + 1].hw >> 4) & 3) == (seq_pos(simd) + 1) % 4; }
        }
    }
    // per CU: the starts of its workgroups, and which bit fields of blockIdx.x number them
    std::map<int, int> n_per_cu, distinct_starts, distinct_starts_together;
    long cu_together = 0, cu4 = 0, field_ok[16] = {0}, delta_rot[4] = {0}, delta_all = 0;
    uint32_t diff_or = 0, diff_and = ~0u;
    for (auto &kv : percu) {
        std::vector<int> &wgs = kv.second;
        std::sort(wgs.begin(), wgs.end());
        n_per_cu[(int)wgs.size()]++;
        uint32_t seen = 0;
        for (int b : wgs) seen |= 1u << seq_pos((h[(size_t)b * waves].hw >> 4) & 3);
        uint64_t cu_in = 0, cu_out = ~0ull;   // (s_memtime: one clock within a CU)
        for (int b : wgs)
            for (int w = 0; w < waves; ++w) { cu_in = std::max(cu_in, h[(size_t)b * waves + w].t0); cu_out = std::min(cu_out, h[(size_t)b * waves + w].t1); }
        cu_together += cu_in < cu_out;
        if (cu_in < cu_out) distinct_starts_together[__builtin_popcount(seen)]++;
        distinct_starts[__builtin_popcount(seen)]++;
        for (size_t i = 0; i + 1 < wgs.size(); ++i) {   // how far the start moves from one workgroup of the CU to the next (in positions of the cyclic order)
            const int p0 = seq_pos((h[(size_t)wgs[i] * waves].hw >> 4) & 3), p1 = seq_pos((h[(size_t)wgs[i + 1] * waves].hw >> 4) & 3);
            delta_rot[(p1 - p0 + 4) & 3]++; ++delta_all;
            diff_or |= (uint32_t)(wgs[i] ^ wgs[i + 1]); diff_and &= (uint32_t)(wgs[i] ^ wgs[i + 1]);
        }
        if (wgs.size() == 4) {
            ++cu4;
            for (int sh = 0; sh < 16; ++sh) {
                uint32_t m = 0;
                for (int b : wgs) m |= 1u << ((b >> sh) & 3);
                field_ok[sh] += m == 0xFu;
            }
        }
    }
    fprintf(f, "  {\"waves_per_workgroup\": %d, \"threads\": %d, \"launch_bounds\": \"%s\", \"lds_bytes\": %zu, \"grid\": %d, \"spins\": %d,\n", waves, waves * 64,
            waves <= 8 ? "512, 8" : "1024, 4", lds, kGrid, spins);
    fprintf(f, "   \"realtime_ticks\": {\"first_entry\": 0, \"last_entry\": %llu, \"first_exit\": %llu, \"last_exit\": %llu}, \"grid_co_resident\": %s,\n",
            (unsigned long long)(last_in - first_in), (unsigned long long)(first_out - first_in), (unsigned long long)(last_out - first_in), resident ? "true" : "false");
    fprintf(f, "   \"cus_used\": %zu, \"cus_whose_workgroups_all_overlap_in_time\": %ld, \"workgroups_split_over_cus\": %ld, \"cus_by_workgroups_resident\": {", percu.size(),
            cu_together, split);
    { bool c = false; for (auto &kv : n_per_cu) { fprintf(f, "%s\"%d\": %d", c ? ", " : "", kv.first, kv.second); c = true; } }
    fprintf(f, "},\n   \"a_waves_w_and_w_plus_4_share_a_simd\": {\"pairs\": %ld, \"same_simd\": %ld},\n", pair_all, pair_same);
    fprintf(f, "   \"consecutive_waves_follow_0_2_1_3\": {\"pairs\": %ld, \"in_order\": %ld},\n", order_all, order_ok);
    fprintf(f, "   \"b_distinct_start_simds_per_cu\": {");
    { bool c = false; for (auto &kv : distinct_starts) { fprintf(f, "%s\"%d\": %d", c ? ", " : "", kv.first, kv.second); c = true; } }
    fprintf(f, "},\n   \"b_distinct_start_simds_per_cu_where_the_workgroups_all_overlap_in_time\": {");
    { bool c = false; for (auto &kv : distinct_starts_together) { fprintf(f, "%s\"%d\": %d", c ? ", " : "", kv.first, kv.second); c = true; } }
    fprintf(f, "},\n   \"b_start_moves_between_consecutive_workgroups_of_a_cu\": {\"by_0\": %ld, \"by_1\": %ld, \"by_2\": %ld, \"by_3\": %ld, \"pairs\": %ld},\n",
            delta_rot[0], delta_rot[1], delta_rot[2], delta_rot[3], delta_all);
    fprintf(f, "   \"c_blockidx_bits_differing_between_consecutive_workgroups_of_a_cu\": {\"or\": \"0x%x\", \"and\": \"0x%x\"},\n", diff_or, delta_all ? diff_and : 0u);
    fprintf(f, "   \"c_cus_with_4_workgroups\": %ld, \"c_cus_where_blockidx_field_takes_0_to_3\": {", cu4);
    for (int sh = 0; sh < 10; ++sh) fprintf(f, "%s\"(b >> %d) & 3\": %ld", sh ? ", " : "", sh, field_ok[sh]);
    fprintf(f, "},\n   \"cus\": [\n");
    size_t n = 0;
    for (auto &kv : percu) {
        fprintf(f, "    {\"xcc\": %u, \"se\": %u, \"sh\": %u, \"cu\": %u, \"workgroups\": [", kv.first >> 16, (kv.first >> 13) & 7u, (kv.first >> 12) & 1u, (kv.first >> 8) & 15u);
        for (size_t i = 0; i < kv.second.size(); ++i) fprintf(f, "%s%d", i ? ", " : "", kv.second[i]);
        fprintf(f, "], \"simd_of_each_wave\": [");
        for (size_t i = 0; i < kv.second.size(); ++i) {
            fprintf(f, "%s\"", i ? ", " : "");
            for (int w = 0; w < waves; ++w) fprintf(f, "%u", (h[(size_t)kv.second[i] * waves + w].hw >> 4) & 3u);
            fprintf(f, "\"");
        }
        fprintf(f, "]}%s\n", ++n < percu.size() ? "," : "");
    }
    fprintf(f, "   ]}%s\n", last ? "" : ",");
    printf("%d waves: co-resident %d, CUs %zu, w/w+4 same SIMD %ld/%ld, 0-2-1-3 order %ld/%ld, start moves by 0/1/2/3: %ld/%ld/%ld/%ld, diff bits or 0x%x and 0x%x\n", waves,
           (int)resident, percu.size(), pair_same, pair_all, order_ok, order_all, delta_rot[0], delta_rot[1], delta_rot[2], delta_rot[3], diff_or, delta_all ? diff_and : 0u);
    printf("   CUs whose workgroups all overlap: %ld; distinct starts per CU:", cu_together);
    for (auto &kv : distinct_starts) printf(" %d:%d", kv.first, kv.second);
    printf("   fields 0..3 per CU (of %ld):", cu4);
    for (int sh = 0; sh < 10; ++sh) printf(" >>%d:%ld", sh, field_ok[sh]);
    printf("\n");
    return 0;
}

int main(int argc, char **argv)
{
    const char *path = argc > 1 ? argv[1] : "r11_wave_placement.json";
    const int spins = argc > 2 ? atoi(argv[2]) : 50000;   // ~0.75 ms at 8 waves per SIMD: the last workgroup of a launch enters up to 0.45 ms after the first
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    FILE *f = fopen(path, "w");
    if (!f) { perror(path); return 1; }
    fprintf(f, "{\"tool\": \"tools/wave_placement.hip\", \"device\": \"%s\", \"compute_units\": %d,\n", prop.gcnArchName, prop.multiProcessorCount);
    fprintf(f, " \"assumption\": \"the tool's workgroups are assumed to be placed as ladder_wu_kernel's are, because it has the same footprint (threads per workgroup, launch bound, "
               "dynamic LDS of toric L = 9 at the ladder's length, 1024 workgroups); the real kernel's placement is not measured\",\n");
    fprintf(f, " \"hw_id_fields\": \"wave [3:0], simd [5:4], cu [11:8], sh [12], se [15:13]; XCC_ID [3:0]\", \"simd_of_each_wave\": \"one digit per wave of the workgroup, wave 0 first\",\n");
    fprintf(f, " \"shapes\": [\n");
    const int shapes[] = {5, 6, 7, 8, 9};
    for (int i = 0; i < 5; ++i)
        if (run(shapes[i], spins, f, i == 4)) { fclose(f); return 1; }
    fprintf(f, " ]}\n");
    fclose(f);
    return 0;
}
