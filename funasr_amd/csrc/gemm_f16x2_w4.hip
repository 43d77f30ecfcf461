// The f16x2 tile GEMM (gemm_f16x2.hip: C = epilogue(A[M,K] * W[N,K]^T), both operands as two fp16 planes, three
// v_mfma_f32_16x16x32_f16 products per operand pair into one fp32 accumulator) as a FOUR-wave 256 x 256 block: one wave per
// SIMD, each with the SIMD's whole 512-entry register file -- a 128 x 128 output quadrant = 64 accumulator tiles of 16 x 16 = all
// 256 AGPRs, and ONE 32-deep stage's operand fragments (4 kinds x 8 tiles = 128 VGPRs) alive at a time. Same call sites as the
// other shapes (funasr/models/transformer/positionwise_feed_forward.py:14-34, funasr/models/sanm/attention.py:256,306); the same
// products in the same k order per output element and the shared epilogue (gemm_f16x2_epilogue.h), so results are BITWISE those
// of every other shape (tested: tests/test_kernels_f16x2_gpu.py, tests/test_gemm_mfma_shape_gpu.py). Two wave grids over the same K loop:
//   2 x 2: the 256 x 256 tile form (gemm_f16x2.hip's epilogue: fp32 / planes / QKV form), Gemm2Args.tile 7;
//   1 x 4: the 128 x 512 full-row form (gemm_f16x2_row.hip's epilogue: residuals, FSMN memory block, LayerNorm, planes; run once
//          per 64-row half of the block), GemmRowArgs.block_rows 130.
//
// The loop on the 16x16x32 MFMA. A stage is three PRODUCTS of 64 MFMAs, each over the stage's 32 k: lo*hi (A lo x W hi), hi*lo
// (A hi x W lo), hi*hi (A hi x W hi) -- the order of every other shape. Fragment registers are reused as their kind dies: during
// lo*hi the stage's A hi and W lo are read (one ds_read_b128 per four MFMAs); the barrier in front of hi*lo publishes the next stage
// and frees this one's buffer; during hi*lo the NEXT stage's A lo is read (A lo is dead since lo*hi); hi*hi walks the accumulators
// column by column so that W hi tile j is dead after eight MFMAs and the next stage's tile j lands in the same registers. One stage
// per loop iteration and ONE register set: a form with W hi double buffered by stage parity needed two stages per iteration and two
// tails, and the joins of that control flow made the allocator spill the 64 accumulator tuples (1.7 - 2.8 KB of scratch per lane).
// The DMA pieces of the stage after next go out spread over the 64 MFMA gaps of hi*lo and are waited for behind the next lo*hi.
//
// Why another shape (round 5). The eight-wave shapes read ALL fragments of a 32-deep stage right behind the stage's barrier,
// with both waves of every SIMD waiting for them at the same time: 192 ds_read_b128 (768 LDS cycles) per 3072 cycles of
// matrix work run uncovered -- the loop alone reaches 0.62 of the matrix rate (tools/abl_gemm2.py). Here
//   * LDS reads per MFMA drop by a third (16 ds_read_b128 per 48 MFMAs against 12 per 24) and the NEXT k-step's fragments
//     are read under the current k-step's MFMAs, one read per two MFMAs, placed by hand (every instruction of the K loop is
//     issued from volatile asm in source order: with one wave per SIMD nothing else fills the matrix pipe's shadow). The loop
//     alone (no DMA, no epilogue; M = 32768, w_1) runs 92 us on zero operands = 0.90 of the 2.5 PFLOP/s peak, and 124-139 us
//     on random operands = the power-limited rate of this instruction mix (tools/micro/mfma_peak.hip: 1647 TFLOP/s at
//     1.78 GHz / 1240 W; profiles/r05a_w4_first_run.jsonl);
//   * operand staging as in the eight-wave shapes: two 64-KB stages (32 deep, 64-B LDS rows, chunk swizzle c ^ (-(r >> 2) & 3)),
//     every wave issues 16 of a stage's 64 one-KB LDS-DMA pieces, one per three MFMA gaps, during the k-step in which the
//     buffer falls free, and waits for them -- vmcnt(0): the only exact wait on LDS-DMA (DESIGN, round 4) -- a k-step later;
//     ONE barrier per stage, in the middle of it (it publishes the next stage and frees the buffer just read);
//   * measured and dropped on the way (profiles/r05a..c): a ring of four / five 16-deep stages with one owner wave per stage
//     (exact waits with three / four stages in flight). Its cover was never the problem -- four and five stages took the same
//     time -- its cost was the owner's issue burst (32 pieces in one k-step from ONE wave: whatever does not fit an MFMA's
//     shadow idles that SIMD's matrix pipe, and the other three waves wait for the owner at the step's barrier: +50 us on a
//     92-us loop) and the 32-B row slices of a 16-deep stage (twice the address-coalescer work per byte: -12 us with a
//     contiguous pattern). Uniform issue by all waves is what the exact wait allows only with ONE stage in flight.
#include "common.h"
#include "gemm_f16x2_epilogue.h"
#include "gemm_f16x2_row_epilogue.h"

namespace pf {

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// wave grid GM x GN (GM GN == 4), every wave a 128 x 128 quadrant. A 32-deep stage = [A hi | A lo | W hi | W lo] of 64-B rows
template <int GM_, int GN_> struct W4Geo {
    static constexpr int GM = GM_, GN = GN_;
    static constexpr int BM = GM * 128, BN = GN * 128;
    static constexpr int A_PLANE_B = BM * 64, W_PLANE_B = BN * 64;
    static constexpr int STAGE_B = 2 * (A_PLANE_B + W_PLANE_B);      // 64 KB (2 x 2) / 80 KB (1 x 4)
    static constexpr int NPW = STAGE_B / 1024 / 4;                   // 1-KB pieces per wave and stage: 16 / 20
    static constexpr int TA = BM / 64, TW = BN / 64;                 // this wave's pieces per A / W plane: 4 / 2 and 4 / 8
    static constexpr int LDS_B = 2 * STAGE_B;
    static_assert(GM * GN == 4 && NPW == 2 * (TA + TW), "four waves");
};

// a 32-deep stage's fragments: 8 row tiles (A) / 8 column tiles (W) of 16 x 32, lo and hi planes. W hi is used by the first product
// of a stage and by the last, so the next stage's copy needs registers of its own: two sets, by stage parity
struct W4Frags { f16x8 al[8], ah[8], bl[8], bh[8]; };

__device__ __forceinline__ void w4_mfma(floatx4& acc, const f16x8& a, const f16x8& b) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}
template <int OFF> __device__ __forceinline__ void w4_read(f16x8& dst, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}
// every fragment read of this wave has returned; the operands tie the wait to the registers it covers (volatile asm statements keep
// their source order, so the ties that do not fit one statement follow in empty ones)
__device__ __forceinline__ void w4_tie8(f16x8 (&x)[8]) {
    asm volatile("" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]));
}
__device__ __forceinline__ void w4_reads_done(W4Frags& f) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    w4_tie8(f.al); w4_tie8(f.ah); w4_tie8(f.bl); w4_tie8(f.bh);
}
// the compiler does not see an MFMA in w4_mfma: the wait states between the last product (or the zero fill) and the next
// reader of an accumulator are spent here. Sized for the 16 passes of a 32 x 32 x 16 product + the write-back; the 16 x 16 x 32
// product has 8 passes and needs less (11 wait states before a VALU read), so the old size is kept: it runs twice per kernel.
__device__ __forceinline__ void w4_settle(floatx4 (&acc)[8][8]) {
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
    for (int i = 0; i < 8; ++i)
        asm volatile("" : "+a"(acc[i][0]), "+a"(acc[i][1]), "+a"(acc[i][2]), "+a"(acc[i][3]), "+a"(acc[i][4]), "+a"(acc[i][5]), "+a"(acc[i][6]), "+a"(acc[i][7]));
}
// one 1-KB LDS-DMA piece: uniform 64-bit base + 32-bit per-lane byte offset, destination lds_buf + LOFF. No branch, no compare:
// a piece costs the issuing wave ~17 cycles of scalar work and ~19 of VMEM issue that one MFMA's shadow has to hold
// (profiles/r05h_w4_piece_cost_probes.jsonl), so the stages that issue nothing are a separate copy of the loop body.
template <int LOFF, bool NT> __device__ __forceinline__ void w4_piece(const char* sbase, unsigned voff, unsigned lds_buf) {
    if constexpr (NT)
        asm volatile("s_add_u32 m0, %2, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1 nt" : : "v"(voff), "s"(sbase), "s"(lds_buf), "n"(LOFF) : "memory", "scc");
    else
        asm volatile("s_add_u32 m0, %2, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(sbase), "s"(lds_buf), "n"(LOFF) : "memory", "scc");
    // (m0 is reserved: the compiler keeps nothing in it)
}

// The K loop of both forms: acc += A[m0 .., :] W[n0 .., :]^T over p.K (a multiple of 32, >= 64), this wave's quadrant (wr, wc).
// NODMA (timing only): 1 = no LDS-DMA pieces and no waits for them (the MFMA + fragment-read loop alone)
template <class G, int NODMA, bool A_NT>
__device__ __forceinline__ void w4_kloop(const unsigned short* A, int lda, size_t a_plane, const unsigned short* W, int ldw, size_t w_plane,
                                         int M, int N, int K, int m0, int n0, unsigned char* smem, int wave, int wr, int wc, int lane,
                                         floatx4 (&acc)[8][8]) {
    const int q16 = lane >> 4, l16 = lane & 15;
    // ---- DMA sources. A stage is STAGE_B / 1024 pieces of 16 rows x 64 B of one plane (lane l -> row l / 4, physical chunk l % 4
    //      <- the logical chunk the read-side swizzle expects there), linear in LDS; wave w issues pieces w + 4 i: the A planes'
    //      row groups 16 (w + 4 t) .. first, then the W planes'
    unsigned va[G::TA], vw[G::TW];
    {
        const int prow = lane >> 2;
        const unsigned chunkb = (unsigned)(((lane & 3) ^ ((0 - (prow >> 2)) & 3)) * 16);      // the swizzle of the 16x16x32 fragment read
#pragma unroll
        for (int t = 0; t < G::TA; ++t) {
            int row = m0 + 16 * (wave + 4 * t) + prow;
            row = row < M ? row : M - 1;
            va[t] = (unsigned)row * (unsigned)lda * 2u + chunkb;
        }
#pragma unroll
        for (int t = 0; t < G::TW; ++t) {
            int col = n0 + 16 * (wave + 4 * t) + prow;
            col = col < N ? col : N - 1;
            vw[t] = (unsigned)col * (unsigned)ldw * 2u + chunkb;
        }
    }
    const char* const a_hi = reinterpret_cast<const char*>(A);
    const char* const a_lo = a_hi + a_plane * 2;
    const char* const w_hi = reinterpret_cast<const char*>(W);
    const char* const w_lo = w_hi + w_plane * 2;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
    const unsigned ldsw = lds0 + (unsigned)wave * 1024;
    // this wave's piece I (0 .. NPW - 1) of stage `js` -> the stage buffer at byte address `buf` (+ wave KB)
    auto piece = [&](auto I, int js, unsigned buf) {
        constexpr int i = decltype(I)::value;
        if constexpr (NODMA == 1) return;
        const size_t ko = (size_t)js * 64;
        if constexpr (i < G::TA) w4_piece<4096 * i, A_NT>(a_hi + ko, va[i], buf);
        else if constexpr (i < 2 * G::TA) w4_piece<G::A_PLANE_B + 4096 * (i - G::TA), A_NT>(a_lo + ko, va[i - G::TA], buf);
        else if constexpr (i < 2 * G::TA + G::TW) w4_piece<2 * G::A_PLANE_B + 4096 * (i - 2 * G::TA), false>(w_hi + ko, vw[i - 2 * G::TA], buf);
        else w4_piece<2 * G::A_PLANE_B + G::W_PLANE_B + 4096 * (i - 2 * G::TA - G::TW), false>(w_lo + ko, vw[i - 2 * G::TA - G::TW], buf);
    };

    // ---- fragment addresses (operand lane map of the 16x16x32 MFMA): lane l reads row l & 15 of a 16-row tile, logical chunk l >> 4
    //      (k = 8 (l >> 4) .. + 7) of the 64-B row, physical chunk c ^ (-(row >> 2) & 3) (gemm_f16x2.hip)
    const unsigned coff16 = (unsigned)((q16 ^ ((0 - (l16 >> 2)) & 3)) * 16);
    const unsigned fa0 = lds0 + (unsigned)((wr * 128 + l16) * 64) + coff16;
    const unsigned fb0 = lds0 + 2 * G::A_PLANE_B + (unsigned)((wc * 128 + l16) * 64) + coff16;

    const int ns = K / 32;                        // stages (>= 2)

    // ---- prologue: stage 0 lands and is published; the operands of its first product are read; stage 1 is on its way
    [&]<int... I>(std::integer_sequence<int, I...>) { (piece(std::integral_constant<int, I>{}, 0, ldsw), ...); }(std::make_integer_sequence<int, G::NPW>{});
    if constexpr (NODMA == 0) glds_wait_all();
    __builtin_amdgcn_s_barrier();
    W4Frags f;
    [&]<int... T>(std::integer_sequence<int, T...>) { (w4_read<G::A_PLANE_B + T * 1024>(f.al[T], fa0), ...); }(std::make_integer_sequence<int, 8>{});
    [&]<int... T>(std::integer_sequence<int, T...>) { (w4_read<T * 1024>(f.bh[T], fb0), ...); }(std::make_integer_sequence<int, 8>{});
    [&]<int... I>(std::integer_sequence<int, I...>) { (piece(std::integral_constant<int, I>{}, 1, ldsw + G::STAGE_B), ...); }(std::make_integer_sequence<int, G::NPW>{});
    w4_reads_done(f);

#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;
    w4_settle(acc);

    // ---- one product of a stage (parity P): 64 MFMAs over the stage's 32 k, consecutive ones on different accumulators.
    //      PH 0: lo * hi (A lo x W hi[P]) while A hi and W lo of the SAME stage are read from (fa, fb), one read per four MFMAs;
    //      PH 1: hi * lo (A hi x W lo) while the NEXT stage's A lo is read from (fa, fb) -- A lo is dead since PH 0;
    //      PH 2: hi * hi (A hi x W hi[P]) while the NEXT stage's W hi is read into the other set, one read per eight MFMAs.
    //      ISSUE: this wave's pieces of stage `js` go out, spread evenly over the 64 MFMA gaps of PH 1, so that each has PH 2 and the
    //      next stage's PH 0 (128 MFMAs, as long as the 48 of a 16-deep step of the 32x32 form) to land before it is waited for
    auto product = [&](auto Ph, auto Issue, unsigned fa, unsigned fb, int js, unsigned buf) {
        constexpr int PH = decltype(Ph)::value;
        constexpr bool ISSUE = decltype(Issue)::value;
        [&]<int... Gp>(std::integer_sequence<int, Gp...>) {
            ([&] {
                // PH 0 / 1 walk the accumulators row by row; PH 2 column by column, so that W hi tile j is dead after eight MFMAs
                // and the next stage's tile j can land in the same registers (read one MFMA into the next column)
                constexpr int g = Gp, i = PH == 2 ? (g & 7) : (g >> 3), j = PH == 2 ? (g >> 3) : (g & 7);
                if constexpr (PH == 0) w4_mfma(acc[i][j], f.al[i], f.bh[j]);
                else if constexpr (PH == 1) w4_mfma(acc[i][j], f.ah[i], f.bl[j]);
                else w4_mfma(acc[i][j], f.ah[i], f.bh[j]);
                if constexpr (PH == 0 && (g & 3) == 0) {
                    constexpr int r = g >> 2;
                    if constexpr (r < 8) w4_read<r * 1024>(f.ah[r], fa);
                    else w4_read<G::W_PLANE_B + (r - 8) * 1024>(f.bl[r - 8], fb);
                }
                if constexpr (PH == 1 && (g & 7) == 0) w4_read<G::A_PLANE_B + (g >> 3) * 1024>(f.al[g >> 3], fa);
                if constexpr (PH == 2 && (g & 7) == 0 && g >= 8) w4_read<((g >> 3) - 1) * 1024>(f.bh[(g >> 3) - 1], fb);
                // piece q goes behind MFMA (64 q) / NPW + 1 of hi*lo: g carries piece q iff that holds for q = ((g - 1) NPW + 63) / 64
                if constexpr (ISSUE && PH == 1 && g >= 1) {
                    constexpr int q = ((g - 1) * G::NPW + 63) / 64;
                    if constexpr (q < G::NPW && (64 * q) / G::NPW + 1 == g) piece(std::integral_constant<int, q>{}, js, buf);
                }
            }(), ...);
        }(std::make_integer_sequence<int, 64>{});
        if constexpr (PH == 2) w4_read<7 * 1024>(f.bh[7], fb);
    };
    typedef std::integral_constant<int, 0> I0;
    typedef std::integral_constant<int, 1> I1;
    typedef std::integral_constant<int, 2> I2;
    auto stage = [&](auto Issue, int j) {
        const unsigned cur = (unsigned)(j & 1) * G::STAGE_B, nxt = G::STAGE_B - cur;
        product(I0{}, std::false_type{}, fa0 + cur, fb0 + cur, 0, 0u);
        w4_reads_done(f);
        if constexpr (NODMA == 0) glds_wait_all();
        __builtin_amdgcn_s_barrier();
        product(I1{}, Issue, fa0 + nxt, fb0 + nxt, j + 2, ldsw + cur);
        product(I2{}, Issue, fa0 + nxt, fb0 + nxt, j + 2, ldsw + cur);
        w4_reads_done(f);
    };
    for (int j = 0; j < ns - 2; ++j) stage(std::true_type{}, j);
    stage(std::false_type{}, ns - 2);
    stage(std::false_type{}, ns - 1);             // (reads one stage past the end into A lo / W hi: never multiplied)
    w4_settle(acc);
}

// EABL: the shared epilogue's measurement switch (0 product, 1 no global stores, 2 no epilogue)
template <int MODE, int OUT, int EABL, int NODMA>
__global__ __launch_bounds__(256, 1) void gemm_f16x2_w4_kernel(Gemm2Args p, int nM, int nN) {
    typedef W4Geo<2, 2> G;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int L = blockIdx.x;
    const int xcd = L & 7, j8 = L >> 3;
    const int mblk = (j8 / nN) * 8 + xcd, nblk = j8 % nN;
    if (mblk >= nM) return;
    const int m0 = mblk * G::BM, n0 = nblk * G::BN;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    floatx4 acc[8][8];
    w4_kloop<G, NODMA, false>(p.A, p.lda, p.a_plane, p.W, p.ldw, p.w_plane, p.M, p.N, p.K, m0, n0, smem, wave, wr, wc, lane, acc);
    gemm2_epilogue<4, 4, 4, MODE, OUT, EABL>(p, acc, smem, m0, n0, nblk, wave, wr, wc, lane);
}

#if defined(PF_MEASUREMENT_KERNELS)
// full-row form (N == 512): one workgroup = 128 complete rows, wave w = columns 128 w ..; the row epilogue runs once per 64-row half
template <int MODE, bool LN, bool A_NT>
__global__ __launch_bounds__(256, 1) void gemm_f16x2_w4_row_kernel(GemmRowArgs p) {
    typedef W4Geo<1, 4> G;
    static_assert(G::LDS_B == RW_LDS_B && G::BM == RW_BM && G::BN == RW_BN, "the row epilogue's LDS plan");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int m0 = blockIdx.x * G::BM;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    floatx4 acc[8][8];
    w4_kloop<G, 0, A_NT>(p.A, p.lda, p.a_plane, p.W, p.ldw, p.w_plane, p.M, G::BN, p.K, m0, 0, smem, wave, 0, wave, lane, acc);
    gemm2_row_epilogue<MODE, LN, 256, 4, 0>(p, acc, smem, m0, tid, wave, 0, wave, lane, true);
    gemm2_row_epilogue<MODE, LN, 256, 4, 2>(p, acc, smem, m0, tid, wave, 1, wave, lane, false);
}

#endif

template <int MODE, int OUT, int EABL = 0, int NODMA = 0>
int launch_w4(const Gemm2Args& a, hipStream_t stream) {
    typedef W4Geo<2, 2> G;
    static PerDeviceOnce configured;
    if (!configured.done()) {
        PF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_f16x2_w4_kernel<MODE, OUT, EABL, NODMA>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS_B));
        configured.mark();
    }
    const int nM = ceil_div(a.M, G::BM), nN = ceil_div(a.N, G::BN);
    const int nMpad = (nM + 7) / 8 * 8;
    hipLaunchKernelGGL((gemm_f16x2_w4_kernel<MODE, OUT, EABL, NODMA>), dim3((unsigned)nMpad * nN), dim3(256), G::LDS_B, stream, a, nM, nN);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}

#if defined(PF_MEASUREMENT_KERNELS)
template <int MODE, bool LN, bool A_NT>
int launch_w4_row_t(const GemmRowArgs& a, hipStream_t stream) {
    typedef W4Geo<1, 4> G;
    static PerDeviceOnce configured;
    if (!configured.done()) {
        PF_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_f16x2_w4_row_kernel<MODE, LN, A_NT>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS_B));
        configured.mark();
    }
    hipLaunchKernelGGL((gemm_f16x2_w4_row_kernel<MODE, LN, A_NT>), dim3((unsigned)ceil_div(a.M, G::BM)), dim3(256), G::LDS_B, stream, a);
    PF_HIP_TRY(hipGetLastError());
    return 0;
}
template <int MODE, bool LN>
int launch_w4_row_m(const GemmRowArgs& a, hipStream_t stream) {
    return (a.a_nt & 1) ? launch_w4_row_t<MODE, LN, true>(a, stream) : launch_w4_row_t<MODE, LN, false>(a, stream);
}

#endif

}  // namespace

bool gemm_f16x2_w4_ok(const Gemm2Args& a) {
    // rows / columns are clamped in the DMA sources and masked in the epilogue like the other shapes; 32-bit per-lane byte offsets
    // (not the QKV / KV form: its epilogue on top of 256 accumulator registers spills -- 326 us against the eight-wave shape's 177 at
    // the headline shape before the 16x16x32 loop, more behind it; that form is chosen by shape)
    return a.qkv_D <= 0 && a.K % 32 == 0 && a.K >= 64 && a.N % 256 == 0 && a.kslices <= 1 && a.ksplit <= 1 && !a.amax_val && a.a_kstep <= 0 && a.w_kstep <= 0 &&
           (size_t)a.M * (size_t)a.lda * 2 < (1ull << 32) && (size_t)a.N * (size_t)a.ldw * 2 < (1ull << 32);
}

// abl (measurement only): 0 product, 1 no global stores, 2 no epilogue, 3 no epilogue and no operand DMA (the loop alone)
int launch_gemm_f16x2_w4(const Gemm2Args& a, int abl, hipStream_t stream) {
    PF_REQUIRE(gemm_f16x2_w4_ok(a), "gemm_f16x2 (four-wave shape): needs K % 32 == 0, K >= 64, N % 256 == 0 and operands below 4 GB");
    const int mode = (a.R1 ? 1 : 0) | (a.R2 ? 2 : 0);
    if (a.C2) {
        PF_REQUIRE(mode == 0, "gemm_f16x2: the plane output has no residual form");
#if defined(PF_MEASUREMENT_KERNELS)
        if (abl == 1) return launch_w4<0, 1, 1>(a, stream);
#endif
        return launch_w4<0, 1>(a, stream);
    }
#if defined(PF_MEASUREMENT_KERNELS)
    if (abl == 1) return launch_w4<0, 0, 1>(a, stream);
    if (abl == 2) return launch_w4<0, 0, 2>(a, stream);
    if (abl == 3) return launch_w4<0, 0, 2, 1>(a, stream);
#else
    PF_REQUIRE(abl == 0, "gemm_f16x2 (four-wave shape): the ablation builds are in the measurement library (make measure)");
#endif
    switch (mode) {
        case 0: return launch_w4<0, 0>(a, stream);
        case 1: return launch_w4<1, 0>(a, stream);
        case 2: return launch_w4<2, 0>(a, stream);
        default: return launch_w4<3, 0>(a, stream);
    }
}

bool gemm_f16x2_w4_row_ok(const GemmRowArgs& a) {
    return a.N == 512 && a.K % 32 == 0 && a.K >= 64 && (size_t)a.M * (size_t)a.lda * 2 < (1ull << 32) && (size_t)a.ldw * 1024 < (1ull << 32);
}

// the four-wave full-row form (measurement library only); the caller (launch_gemm_f16x2_row) has checked the arguments
#if defined(PF_MEASUREMENT_KERNELS)
int launch_gemm_f16x2_w4_row(const GemmRowArgs& a, hipStream_t stream) {
    PF_REQUIRE(gemm_f16x2_w4_row_ok(a), "gemm_f16x2_row (four-wave shape): needs N == 512, K % 32 == 0, K >= 64 and operands below 4 GB");
    const bool ln = a.ln_g != nullptr;
    if (a.fs_v) return a.R2 ? launch_w4_row_m<6, true>(a, stream) : launch_w4_row_m<4, true>(a, stream);
    const int mode = (a.R1 ? 1 : 0) | (a.R2 ? 2 : 0);
    switch (mode * 2 + (ln ? 1 : 0)) {
        case 0: return launch_w4_row_m<0, false>(a, stream);
        case 1: return launch_w4_row_m<0, true>(a, stream);
        case 2: return launch_w4_row_m<1, false>(a, stream);
        case 3: return launch_w4_row_m<1, true>(a, stream);
        case 4: return launch_w4_row_m<2, false>(a, stream);
        case 5: return launch_w4_row_m<2, true>(a, stream);
        case 6: return launch_w4_row_m<3, false>(a, stream);
        default: return launch_w4_row_m<3, true>(a, stream);
    }
}

#else
int launch_gemm_f16x2_w4_row(const GemmRowArgs&, hipStream_t) {
    set_error("gemm_f16x2_row (four-wave shape): measured and off -- in the measurement library only (make measure)");
    return -1;
}
#endif

}  // namespace pf
