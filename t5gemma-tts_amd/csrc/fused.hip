// The persistent decode launches' host side and primary translation unit: the launcher of every
// variant, the one-tile bf16 kernels (fused_mlp_kernel<1, 2>, fused_block_kernel<0..2>; the code
// is fused_kernels.h and the stage headers it includes) and the diagnostic symbols of the
// T5G_DBG_TS library.
//
// The two-tile (17-32 row) instantiations of fused_block_kernel are compiled as a translation
// unit of their own (fused_rows32.hip): instantiated beside the one-tile kernels they change the
// compiler's inlining decisions for those, and the one-tile kernels stay the code they were.
// The FP8 (P8, fp8.h) instantiations of the one-tile kernels are a third translation unit for
// the same reason (fused_p8.hip), and the P8 instantiations of fused_mlp_kernel a fourth
// (fused_mlp_p8.hip). They carry kernels only, so the four units must stay separately compiled;
// the launcher and the diagnostic symbols stay here.
#include "common.h"

namespace t5g {
T5G_TS_UNIT(fused)
// diagnostic timeline of stage S and O1 (fused_attn.h FS_TS; tools/diag_fused_s.py). This unit
// owns the symbols (T5G_FUSED_DIAG); in the other two the points compile to nothing.
#if defined(T5G_DBG_TS)
__device__ unsigned long long* fs_ts_buf;
extern "C" int t5g_dbg_set_fused_s(void* p) {
    return hipMemcpyToSymbol(HIP_SYMBOL(fs_ts_buf), &p, sizeof(p)) == hipSuccess ? 0 : -1;
}
// timing variants of stage S (never in the product): 1 no K / V loads, 2 one q|k|v slab
// address for every lane, 3 every (row, kv head) reads row 0 / kv head 0's cache (L2 hits),
// 4 the stage run twice (the second one warm: instruction cache, TLB, L2), 5 no K / V load
// instructions at all
__device__ int fs_dbg_var;
extern "C" int t5g_dbg_set_fused_s_var(int v) {
    return hipMemcpyToSymbol(HIP_SYMBOL(fs_dbg_var), &v, sizeof(v)) == hipSuccess ? 0 : -1;
}
#define T5G_FUSED_DIAG 1
#endif
}  // namespace t5g

#include "fused_kernels.h"

namespace t5g {

fused_block_fn fused_block_rows32_kernel(int sv);   // fused_rows32.hip
fused_block_fn fused_block_p8_kernel(int sv);       // fused_p8.hip
typedef void (*fused_mlp_fn)(FusedMlpArgs);
fused_mlp_fn fused_mlp_p8_kernel(int MT);           // fused_mlp_p8.hip

constexpr size_t FM_LDS_MAX = 160 * 1024;

// stage S's arguments, front (self_attn) or tail (self_tail): 8 q heads over 4 kv heads of 256
// (O1's 4 k-slices = the 4 head pairs), the flash kernel's chunk records (rows of <= s_nsplit x
// 64 keys, checked by the host)
static bool stage_s_args_ok(const FusedMlpArgs& a) {
    return a.sk && a.sv && a.kv_len && a.fpart && a.fstat && a.fticket && a.Hq == 8 && a.Hkv == 4 && a.D == FS_D &&
           a.M <= FS_MAXROWS && a.qkv_dim == a.q_dim + 2 * a.Hkv * a.D && a.s_cap >= 1 && a.s_nsplit >= 1 &&
           a.s_nsplit <= DEC_MAX_CHUNKS && a.s_nsplit <= (a.s_cap + FS_CH - 1) / FS_CH && a.window >= 0 &&
           (long)a.M * a.Hkv * a.s_nsplit * FS_G * FS_D * 4 <= 0x7fff0000L;
}

// The dynamic-LDS attribute and the occupancy check of kernel `fn`, once per (device, kernel):
// `done` is the caller's flag for the pair (an engine per GPU in one process must not skip the
// second device's hipFuncSetAttribute). False when the kernel cannot be resident with `shm` bytes.
static bool kernel_ready(const void* fn, size_t shm, bool& done) {
    if (done) return true;
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FM_LDS_MAX);
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, FM_NW * 64, shm) != hipSuccess || occ < 1) return false;
    return done = true;
}

static int fused_mlp_launch(const FusedMlpArgs& a_in, hipStream_t st, bool launch);
int fused_mlp(const FusedMlpArgs& a_in, hipStream_t st) { return fused_mlp_launch(a_in, st, true); }
int fused_mlp_check(const FusedMlpArgs& a_in) { return fused_mlp_launch(a_in, nullptr, false); }

static int fused_mlp_launch(const FusedMlpArgs& a_in, hipStream_t st, bool launch) {
    FusedMlpArgs a = a_in;
    if (a.M <= 0) return 0;
    // the shapes the stages are built for: K = 2304 gate/up (72 k-steps), f = 9216 down in
    // 8 slices of 36 k-steps, 4 cross-o slabs, <= 32 rows
    if (a.M > 32 || a.d != 2304 || a.f != 9216 || a.f % 64) return -1;
    if (!a.part_in || !a.post_w || !a.pre_w || !a.h || !a.xn || !a.Wgu || !a.act || !a.Wd || !a.part_out || !a.sync ||
        !a.sync_next || !a.timeout || a.sync_next == a.sync)
        return -1;
    if (a.NGgu * 8 != a.f || a.NGd * 16 != a.d) return -1;
    // P8 weights, every weight of the launch with its row scales: the MLP-half kernels at one
    // or two tiles (gate/up and down), the whole-layer kernels at one tile only (there is no
    // two-tile P8 block)
    if (a.wfmt != 0 && (a.wfmt != 1 || !a.sWgu || !a.sWd)) return -1;
    if (a.wfmt != 0 && a.xattn &&
        (a.M > 16 || !a.sWq || !a.sWo || (a.Wo1 && !a.sWo1) || (a.Wqkv && !a.sWqkv) || (a.self_tail && !a.sWo1n)))
        return -1;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev))
        return -2;
    const int nb = a.grid > 0 ? a.grid : cus;
    if (nb > cus || nb < FM_DS || nb < a.M) return -1;   // every workgroup must be resident at once
    const int nr = nb - a.M, rest = a.NGgu - a.M * FM_NORM_UNITS;
    if (nr <= 0 || rest < 0) return -1;
    const int nu_g = (rest + nr - 1) / nr;
    const int nu_d = (a.NGd + nb / FM_DS - 1) / (nb / FM_DS);
    if (nu_g > 5 || nu_d > 5) return -1;   // UMAX = 5 batches per wave (needs >= 231 workgroups)
    const int MT = a.M > 16 ? 2 : 1;
    if (a.xattn) {
        // the cross-attention chain: 2 k-slices x NGq cross-q units = one unit-slice per
        // workgroup, 4 x 64 cross-o workgroups, 8 x 32 down workgroups; one 64-key chunk of
        // text keys; attention and norm workgroups disjoint. 17-32 rows (two tiles): a norm
        // workgroup per two rows and an attention workgroup per (row, kv head) with its two q
        // heads, so the same unit limits hold (nw >= 240 of 256)
        const int nn = (a.M + MT - 1) / MT;
        const int nw = nb - nn;   // workers (the last nn workgroups run the norms)
        const int atasks = MT == 2 ? a.M * a.Hkv : a.M * a.Hq;
        if (MT == 2 && a.Hq != 2 * a.Hkv) return -1;
        auto most = [](int units, int per) { return per > 0 ? (units + per - 1) / per : 1 << 20; };
        if (most(a.NGq, nw / 2) > 2 || most(a.NGo, nw / 4) > 3 || most(a.NGd, nw / FM_DS) > 5 ||
            most(a.NGgu, nw) > 5 || (a.Wqkv && most(a.NGqkv, nw / 2) > 3))
            return -1;
        if (a.D != 256 || a.Hq * a.D != a.q_dim || a.Hq % a.Hkv || a.Hq > 8 ||
            a.NGq * 16 != a.q_dim || a.NGo * 16 != a.d || a.text_max > 64 || a.text_max > a.kv_cap || atasks > nw || !a.o_slabs ||
            !a.post1_w || !a.pre1_w || !a.xn1 || !a.Wq || !a.qslab || !a.ck || !a.cv || !a.enc_len || !a.rope_tab ||
            !a.att || !a.Wo || !a.oslab)
            return -1;
        if (!a.dslab || !a.post3_w || !a.pre3_w) return -1;
        if (a.Wo1 && (!a.att_self || !a.o1slab)) return -1;
        // stage S in front: its slabs from the previous launch, <= 3 chunks per workgroup and pass
        if (a.self_attn && (!a.Wo1 || !a.qkv_in || !stage_s_args_ok(a) ||
                            a.M * a.Hkv * a.s_nsplit > FS_GRP * nb * FS_MAXPASS))
            return -1;
        if (a.Wqkv && (!a.qkv_out || a.NGqkv * 16 != a.qkv_dim)) return -1;
        a.norm_b0 = nb - nn;
        static_assert(FB_LDS2 <= FM_LDS_MAX && sizeof(FbSelfLds) <= 2 * 5 * FM_NW * 1024, "two-tile LDS");
        static_assert(FB_GU_KB == FM_NW * 6 && FB_GU_KB % 3 == 0 && FB_LDS <= FM_LDS_MAX, "gate/up LDS unit");
        if (a.d != FB_D) return -1;
        const size_t shm = MT == 2 ? FB_LDS2 : FB_LDS;
        if (dev < 0 || dev >= 64) return -1;
        // the tail: the next layer's S after the q|k|v stage, then its O1 (front O1 off); slots
        // on groups 0-1 of the workers only (group 2 polls), the S scratch in the gate/up unit's LDS
        static_assert(sizeof(FbSelfLds) <= (size_t)FB_GU_KB * 1024, "tail S scratch in the gate/up unit LDS");
        if (a.self_tail && (a.self_attn || a.Wo1 || !a.Wqkv || !a.Wo1n || !a.o1n || !a.att_self ||
                            a.qkv_in != a.qkv_out || !stage_s_args_ok(a) || a.M * a.Hkv * a.s_nsplit > 2 * nw))
            return -1;
        const int sv = a.self_tail ? 2 : a.self_attn ? 1 : 0;
        const int fi = a.wfmt ? 2 : MT - 1;   // kernel family: one tile, two tiles, one tile P8
        fused_block_fn fb = a.wfmt ? fused_block_p8_kernel(sv)
                            : MT == 2 ? fused_block_rows32_kernel(sv)
                            : sv == 2 ? fused_block_kernel<2> : sv ? fused_block_kernel<1> : fused_block_kernel<0>;
        static bool attr_b[64][3][3] = {};
        if (!kernel_ready((const void*)fb, shm, attr_b[dev][fi][sv])) return -1;
        if (!launch) return 0;
        hipLaunchKernelGGL(fb, dim3((unsigned)nb), dim3(FM_NW * 64), shm, st, a);
        return hipGetLastError() == hipSuccess ? 0 : -2;
    }
    const size_t shm = (size_t)5 * MT * FM_NW * 64 * 16;
    if (shm > FM_LDS_MAX) return -1;
    // norm rows on workgroups with one gate/up unit fewer (their weight stream starts after
    // the norm): the last ones
    a.norm_b0 = nb - a.M;
    fused_mlp_fn fn = a.wfmt ? fused_mlp_p8_kernel(MT) : MT == 1 ? fused_mlp_kernel<1> : fused_mlp_kernel<2>;
    if (dev < 0 || dev >= 64) return -1;
    static bool attr[64][2][2] = {};   // (device, format, tiles)
    if (!kernel_ready((const void*)fn, shm, attr[dev][a.wfmt ? 1 : 0][MT - 1])) return -1;
    if (!launch) return 0;
    hipLaunchKernelGGL(fn, dim3((unsigned)nb), dim3(FM_NW * 64), shm, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace t5g
