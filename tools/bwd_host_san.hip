// Stand-alone host program: the pure host helpers of csrc/agg_bwd.hip (bwd_layout, bwd_carve, param_sizes, carve_tensors,
// step_layout, adam_scalars) over the shapes of tests/test_bwd_sizes_cabi.py, meant for a sanitizer build of the HOST code.
// Regions 256-B aligned, in order, ending at `total`; carved pointers at their offsets, first and last byte of every region
// written inside a real allocation.  No GPU is touched: run it on the build machine.
//   hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -O1 -g \
//         -std=c++17 -Iinclude -Idsmil-wsi_amd/csrc tools/bwd_host_san.hip -o /tmp/bwd_host_san \
//         -Ldsmil-wsi_amd -ldsmil_hip -Wl,-rpath,$PWD/dsmil-wsi_amd && /tmp/bwd_host_san
// (the library supplies the forward's symbols agg_bwd.hip refers to; the helpers under test are this unit's own copy)
#include "agg_bwd.hip"
#include <cstdio>
#include <cstdlib>
#include <vector>

static long long checks = 0, fails = 0;
#define CHECK(c) do { ++checks; if (!(c)) { ++fails; std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static void check_layout(int n_bags, long long N, int K, int Kv, int C, int nl) {
    const BwdWs L = bwd_layout(n_bags, N, K, Kv, C, nl);
    const size_t offs[] = {L.gB, L.Dv, L.zero, L.qmax, L.gq, L.gA, L.gs, L.gz2, L.Hb, L.Qb, L.gH, L.gqp, L.wsplit, L.w2t,
                           L.part0, L.part1, L.pb0, L.pb1, L.part, L.part_b, L.off, L.rowbag, L.total};
    const int n = sizeof(offs) / sizeof(offs[0]);
    CHECK(offs[0] == 0);
    for (int i = 0; i < n; ++i) CHECK(offs[i] % 256 == 0);
    for (int i = 0; i + 1 < n; ++i) {
        const bool may_be_empty = (i == n - 2 && n_bags == 0);   // rowbag of the one bag
        CHECK(may_be_empty ? offs[i] <= offs[i + 1] : offs[i] < offs[i + 1]);
    }
    // minimal sizes of the regions whose multiplicity differs between the two forms
    const size_t sets = n_bags ? n_bags : 1;
    CHECK(L.Dv - L.gB >= sets * C * Kv * 4);
    CHECK(L.gq - L.qmax >= sets * C * QD * 4);
    CHECK(L.wsplit - L.gqp >= (size_t)(n_bags ? N / 32 + n_bags + 1 : (N + 31) / 32) * C * QD * 4);
    CHECK(L.total - L.rowbag == (n_bags ? al((size_t)N * 4) : 0));
    CHECK(L.rowbag - L.off == 256);
    CHECK(L.S >= 1 && L.R >= 64 && L.R % 64 == 0 && (long long)L.S * L.R >= N && L.splits >= 1 && L.nx == (K + 63) / 64);
    // the public queries answer a size that fits both forms of the query: the larger of the two layouts
    const size_t answered = n_bags ? dsmil_agg_backward_bags_workspace_bytes(n_bags, N, K, Kv, C) : dsmil_agg_backward_workspace_bytes(N, K, Kv, C);
    const size_t other = bwd_layout(n_bags, N, K, Kv, C, !nl).total;
    CHECK(L.total <= answered && answered == (L.total > other ? L.total : other));
    // the carve: every pointer at its offset; on a real allocation, the first and the last byte of every region are ours
    if (L.total <= (size_t)64 << 20) {
        char* ws = (char*)std::malloc(L.total);
        const BwdBufs b = bwd_carve(ws, L);
        const void* ptrs[] = {b.gB, b.Dv, b.zero, b.qmax, b.gq, b.gA, b.gs, b.gz2, b.Hb, b.Qb, b.gH, b.gqp, b.wsplit, b.w2t,
                              b.part0, b.part1, b.pb0, b.pb1, b.part, b.part_b, b.off, b.rowbag};
        for (int i = 0; i < n - 1; ++i) {
            CHECK((const char*)ptrs[i] == ws + offs[i]);
            if (offs[i + 1] > offs[i]) { ws[offs[i]] = 1; ws[offs[i + 1] - 1] = 2; }
        }
        std::free(ws);
    }
}

int main() {
    const long long rows[] = {1, 31, 32, 33, 64, 65, 65535, 65536, 10000, 640000};
    const int Ks[] = {64, 166, 512, 1024}, Cs[] = {1, 2, 4, 5, 16}, bags[] = {0, 1, 3, 64};
    for (long long N : rows) for (int K : Ks) for (int C : Cs) for (int nl = 0; nl < 2; ++nl) {
        for (int Kv : {K, 96}) for (int nb : bags) if (N >= nb) check_layout(nb, N, K, Kv, C, nl);
        const ParamSizes sz = param_sizes(K, C, nl);
        long long tot = 0;
        for (int i = 0; i < 8; ++i) { CHECK(sz.n[i] >= 0); tot += sz.n[i]; }
        CHECK(tot == sz.total && (sz.n[4] != 0) == (nl != 0) && (sz.n[5] != 0) == (nl != 0) && sz.n[0] == (long long)C * K && sz.n[6] == (long long)C * C * K);
        std::vector<char> buf(8 * 256 + (size_t)sz.total * 4 + 256);
        char* base = (char*)(((uintptr_t)buf.data() + 255) & ~(uintptr_t)255);
        const StepTensors t = carve_tensors(base, sz, nl);
        for (int i = 0; i < 8; ++i) {
            CHECK((uintptr_t)t.t[i] % 256 == 0);
            const char* end = i < 7 ? (const char*)t.t[i + 1] : base + t.bytes;
            CHECK((const char*)t.t[i] + sz.n[i] * 4 <= end);
            if (sz.n[i]) { t.t[i][0] = 1.f; t.t[i][sz.n[i] - 1] = 2.f; }
        }
        CHECK(base + t.bytes <= buf.data() + buf.size());
        CHECK(t.g.fc_w == t.t[0] && t.g.fcc_b == t.t[7] && (t.g.q2_w != nullptr) == (nl != 0) && (t.g.q2_b != nullptr) == (nl != 0));
        // the step layouts end behind their last tensor
        const StepWs s = step_layout(N, K, C, nl);
        CHECK(s.grads % 256 == 0 && s.total == s.grads + t.bytes && s.total == dsmil_agg_train_step_workspace_bytes(N, K, C, nl));
    }
    for (long long step : {1LL, 2LL, 1000LL, 1LL << 40}) {
        const double lr = 1e-4, b1 = 0.5, b2 = 0.9, eps = 1e-8, wd = 1e-3;
        const AdamScalars h = adam_scalars(step, lr, b1, b2, eps, wd);
        CHECK(h.step_size == (float)(lr / (1.0 - pow(b1, (double)step))) && h.w1 == 0.5f && h.beta2 == 0.9f && h.w2 == (float)(1.0 - b2));
        CHECK(h.eps == 1e-8f && h.wd == 1e-3f && h.bc2_sqrt == (float)sqrt(1.0 - pow(b2, (double)step)) && h.bc2_sqrt > 0.f);
    }
    std::printf("%lld checks, %lld failed\n", checks, fails);
    return fails ? 1 : 0;
}
