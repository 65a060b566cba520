// Stand-alone host program: the host code of csrc/stem_bwd.hip (sb_check, sb_plan, the plan and size entries and every refusal of
// dsmil_stem_pool_bwd, none of which launches) over ordinary and extreme shapes, meant for a sanitizer build of the HOST code:
// no signed overflow in the shape arithmetic up to INT32_MAX in every argument, the plan's regions inside the answered size.
// No GPU is touched: run it on the build machine.
//   hipcc --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -O1 -g \
//         -std=c++17 -Iinclude -Idsmil-wsi_amd/csrc tools/stem_bwd_host_san.hip -o /tmp/stem_bwd_host_san && /tmp/stem_bwd_host_san
#include "stem_bwd.hip"
#include <cstdio>

static long long checks = 0, fails = 0;
#define CHECK(c) do { ++checks; if (!(c)) { ++fails; std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

int main() {
    const int dims[] = {-1, 0, 1, 2, 3, 5, 7, 16, 17, 27, 112, 113, 4096, 65535, 65536, 1 << 20, 0x7fffffff};
    const int Cs[] = {-4, 0, 3, 4, 6, 40, 64, 96, 128, 512, 1024, 1536, 2048, 2052, 4096, 0x7fffffff};
    const int Bs[] = {-1, 0, 1, 3, 64, 256, 65536, 0x7fffffff};
    char* const base = (char*)((uintptr_t)1 << 44);          // never dereferenced: every call below is refused before a launch
    for (int B : Bs) for (int H1 : dims) for (int W1 : dims) for (int C : Cs) {
        int32_t plan[16];
        const int rc = dsmil_stem_pool_bwd_plan(B, H1, W1, C, plan);
        const size_t need = dsmil_stem_pool_bwd_workspace_bytes(B, H1, W1, C);
        CHECK((rc == DSMIL_OK) == (need > 0));
        CHECK(rc == DSMIL_OK || rc == DSMIL_E_INVALID || rc == DSMIL_E_UNSUPPORTED);
        CHECK((rc == DSMIL_E_INVALID) == (B < 1 || H1 < 1 || W1 < 1 || C < 1));
        const size_t gap = (size_t)1 << 40;
        const int rcall = dsmil_stem_pool_bwd((const float*)base, (const float*)(base + gap), (const float*)(base + 2 * gap),
                                              (const float*)(base + 3 * gap), (const uint8_t*)(base + 4 * gap), (float*)(base + 5 * gap),
                                              B, H1, W1, C, base + 6 * gap, 0, nullptr);
        if (rc != DSMIL_OK) { CHECK(rcall == rc || rcall == DSMIL_E_INVALID); continue; }
        CHECK(rcall == DSMIL_E_WORKSPACE);                   // a complete call with an empty workspace gets to the last check
        SbPlan p;
        CHECK(sb_plan(B, H1, W1, C, p) && p.total == need && need % 256 == 0);
        CHECK(p.Hp == (H1 + 1) / 2 && p.Wp == (W1 + 1) / 2 && plan[DSMIL_STEM_BWD_PLAN_HP] == p.Hp);
        CHECK(p.chunk >= 256 && p.chunk <= 4096 && (long long)p.chunk * p.nparts >= (long long)H1 * W1);
        CHECK((long long)p.chunk * (p.nparts - 1) < (long long)H1 * W1 && (long long)p.run_len * p.lanes >= (p.chunk < H1 * W1 ? p.chunk : H1 * W1));
        CHECK(p.grid_partial == B * p.nparts && p.grid_finish >= 1 && p.grid_apply >= 1 && p.grid_apply <= 8192);
        CHECK(p.off_coef >= (size_t)2 * B * p.nparts * C * 4 && p.total - p.off_coef >= (size_t)2 * B * C * 4);
    }
    std::printf("%lld checks, %lld failed\n", checks, fails);
    return fails ? 1 : 0;
}
