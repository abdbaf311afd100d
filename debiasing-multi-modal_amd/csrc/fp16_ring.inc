// The fp16 ring of the deep-pipelined 256 x 256 x 64 structure, textually included into gemm_f16_8ph_kernel (f16_ops.hip) and
// pairdist_tile_kernel (pairdist.hip): 512 threads = 8 waves (2 x 4, 128 x 64 of output each), one workgroup per CU.
//   * operands reach LDS by LDS-DMA (buffer_load ... lds, 1 KB per wave instruction): no staging registers, no ds_write; the stager's
//     row / swizzle map is ring_rows (persistent_tiles.h);
//   * a K tile is four HALF-TILES of 128 rows x 64 k (16 KB): Ah0 / Ah1 = the first / second 64 rows of both wave rows' A blocks,
//     Bh0 / Bh1 = the even / odd columns of all four wave columns' B blocks.  A wave walks its 128 x 64 block as four 64 x 32 quadrants,
//     one per PHASE: (A0,B0) (A0,B1) (A1,B1) (A1,B0), so a phase needs at most one new half of each operand (12 / 4 / 8 / 0
//     ds_read_b128) and every half-tile has ONE phase in which it is first needed;
//   * each phase also stages one half-tile (2 DMA instructions per thread) for five phases later; the phase's counted wait (six DMA
//     instructions = three half-tiles stay in flight -- the queue is never drained in the loop) retires the one staged three phases ago, which is read one phase after
//     that wait; a slot is restaged >= 3 phases after its last read.  LDS: [buffer 2][Ah0, Bh0, Bh1, Ah1] = 8 x PH_HALF = 128 KB;
//   * the wave rows run ONE BARRIER APART: while waves 0-3 issue their 8 MFMAs (256 cycles, s_setprio 1) waves 4-7 do their LDS reads,
//     DMA issue and waits, and vice versa -- each SIMD's two waves alternate on the matrix pipe.
// Two K tiles per loop trip.  Expects in scope: lds (8 * PH_HALF bytes, 1024-B aligned), tid, wid, wr, wc, fr, fh and the kernel's
//   ring_src(kind, t, rs, vo, so): half-tile kind (0..3 = Ah0, Bh0, Bh1, Ah1) of K tile t -> buffer descriptor, the thread's two lane
//   offsets and the scalar byte offset of the K tile.  K tiles past the end must still issue (through a zero-extent descriptor, or into
//   buffers no phase reads again): every phase issues exactly two DMA instructions per wave, the vmcnt arithmetic relies on it.
// Defines: acc[4][2] (row block i, column parity j), stage, phase, ring_prologue(tb), ring_item(tb, te, drain, before_trip).

// stage number q: kind q & 3 of K tile q >> 2 into buffer (q >> 2) & 1
auto stage = [&](int kind, int buf, int t) {
    unsigned char* slot = lds + (buf * 4 + kind) * PH_HALF + wid * 1024;
    __amdgpu_buffer_rsrc_t rs;
    unsigned vo[2], so;
    ring_src(kind, t, rs, vo, so);
#pragma unroll
    for (int i = 0; i < 2; ++i) glds16(rs, slot + i * 8192, vo[i], so);
};
// fragment addresses inside a half-tile (bytes): A rows wr * 64 + blk * 32 + fr, B rows wc * 32 + fr, chunk (2 ks + fh) ^ swz
int aoff[2][4], boff[4];
#pragma unroll
for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int r = wr * 64 + b * 32 + fr;
        aoff[b][ks] = r * 128 + (((2 * ks + fh) ^ ((r >> 1) & 7)) << 4);
    }
    const int r = wc * 32 + fr;
    boff[ks] = r * 128 + (((2 * ks + fh) ^ ((r >> 1) & 7)) << 4);
}
f32x16 acc[4][2];
u32x4 fa[2][4], fb0[4], fb1[4];

// one phase: j = phase within the loop trip (static), t2 = first K tile of the trip
// `first`: the item's first trip.  Its prologue has staged both K tiles of the trip (stages 0 .. 7), so phases 0 - 2 stage
// nothing and phases 0 - 4 wait for nothing: the first counted wait (phase 5) is where a previous tile's epilogue stores
// -- older in the queue than every DMA of this tile -- have to be acknowledged, 2000+ cycles after they were issued,
// instead of at the top of the tile.
auto phase = [&](int j, int t2, bool first) {
    const int ph = j & 3, buf = (j >> 2) & 1;
    const unsigned char* base = lds + buf * 4 * PH_HALF;
    if (ph == 0) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) fb0[ks] = *(const u32x4*)(base + 1 * PH_HALF + boff[ks]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) fa[b][ks] = *(const u32x4*)(base + 0 * PH_HALF + aoff[b][ks]);
    } else if (ph == 1) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) fb1[ks] = *(const u32x4*)(base + 2 * PH_HALF + boff[ks]);
    } else if (ph == 2) {
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) fa[b][ks] = *(const u32x4*)(base + 3 * PH_HALF + aoff[b][ks]);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (!(first && j < 3)) {
        const int q = j + 5;                                      // stage number relative to the trip's first tile
        stage(q & 3, (q >> 2) & 1, t2 + (q >> 2));
    }
    __builtin_amdgcn_sched_barrier(0);
    if (!(first && j < 5)) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    const int ai = (ph >= 2) ? 2 : 0, bj = (ph == 1 || ph == 2) ? 1 : 0;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int b = 0; b < 2; ++b)
            acc[ai + b][bj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fa[b][ks]),
                                                                     __builtin_bit_cast(f16x8, bj ? fb1[ks] : fb0[ks]), acc[ai + b][bj], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
};
// prologue of an item whose K tiles start at tb: stages 0 .. 7 = its first two K tiles, both buffers
auto ring_prologue = [&](int tb) {
#pragma unroll
    for (int q = 0; q < 8; ++q) stage(q & 3, (q >> 2) & 1, tb + (q >> 2));
};
// One item: K tiles [tb, te) (both even) into zeroed accumulators; its prologue has been issued.  The prologue's 16 DMA instructions must
// have landed.  drain: wait for everything (nothing but the prologue is outstanding, or the kernel has no epilogue stores); else the 64
// epilogue stores issued AFTER the prologue need not have been acknowledged yet (4.6 us of a GEMM tile's fixed cost when they were waited
// for here): vmcnt(63) leaves at most 63 of the 80 outstanding, i.e. retires the 16 DMAs (and one store).
// before_trip(t2): the kernel's hook ahead of every trip after the first.
auto ring_item = [&](int tb, int te, bool drain, auto&& before_trip) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    if (drain) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(63)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();                    // the second wave row runs one barrier behind
#pragma unroll
    for (int j = 0; j < 8; ++j) phase(j, tb, true);
    for (int t2 = tb + 2; t2 < te; t2 += 2) {
        before_trip(t2);
#pragma unroll
        for (int j = 0; j < 8; ++j) phase(j, t2, false);
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // the look-ahead DMA past the item's last K tile
    __builtin_amdgcn_s_barrier();                                 // every wave is done with the ring
};
