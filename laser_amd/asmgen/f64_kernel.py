"""float64 GEMM kernels for gfx950, hand-scheduled: the f32 generator's program structure (f32_kernel.Gen: 3-stage LDS ring,
one barrier per K-tile, one body per stage, counted waits, accumulators in AGPRs, laser-order fold every kc) with the f64
matrix instruction on the 16x16-block families' padded-row LDS image (gen16x16.Gen16x16, the base class shared with f32x16_kernel).

  v_mfma_f64_16x16x4_f64   16x16 block, 4 k per instruction (64 cycles per SIMD on MI355X), lane l feeds A[l % 16][l / 16] and
                           B[l / 16][l % 16] and holds D[l / 16 + 4 * d][l % 16], d = 0..3: 8 accumulator registers per block
  kc = 256                 gemm_tiling.nim:310 (2048 bytes / sizeof(float64)): the running sum is folded every 16 K-tiles of 16

LDS image (per stage: A panel rows 0..BM-1, then the B panel rows = columns of the tile): a row holds BK = 16 doubles as 8
chunks of 16 bytes, chunk 4*(k / 8) + k % 4 holding k and k + 4 -- the two k-steps lane group q = k % 4 needs from one
ds_read_b128 -- and is 144 bytes long: with 9 chunks per row the 16 rows a 16-lane group reads fall into 16 different
4-bank groups, so the fragment reads are conflict-free without a swizzle, and every store is ONE ds_write2_b64:
  A piece (16 bytes = k0, k0 + 1 of one row)      -> chunks c and c + 1 of that row:           offsets 0, +16 bytes
  B piece (16 bytes = columns x0, x0 + 1 of one k) -> the same chunk of rows x0 and x0 + 1:     offsets 0, +144 bytes
Operands: A row-major (k-contiguous), B row-major (x-contiguous) or passed transposed (`_nt`: k-contiguous, stored like A), C
row-major; K a multiple of 2; any alpha / beta (float64 in the kernel arguments)."""
from .core import v, s, VCC
from .f32_kernel import Cfg, kernel_text, write_kernels, KA_A, KA_LDA  # noqa: F401
from .gen16x16 import Gen16x16

CONFIGS = {
    # one wave per SIMD: 2 x 2 waves of 64x64 = 16 blocks = 128 accumulator registers (+ 128 for the running sum)
    "exact_128x128x16": dict(BM=128, BN=128, BK=16, exact=True, runv=True, dataa=True, pipe=True),
    "fast_128x128x16": dict(BM=128, BN=128, BK=16, exact=False, pipe=True),
    # problems of few tiles (the reference's f64 bench shape, 960^3 = 225 tiles): 2 x 2 waves of 32x32, several workgroups per CU
    "exact_64x64x16": dict(BM=64, BN=64, BK=16, exact=True, runv=True, pipe=True),
    "fast_64x64x16": dict(BM=64, BN=64, BK=16, exact=False, pipe=True),
    # B passed transposed (rowStrideB == 1: k-contiguous like A)
    "exact_128x128x16_nt": dict(BM=128, BN=128, BK=16, exact=True, b_kcontig=True, runv=True, dataa=True, pipe=True),
    "fast_128x128x16_nt": dict(BM=128, BN=128, BK=16, exact=False, b_kcontig=True, pipe=True),
    "exact_64x64x16_nt": dict(BM=64, BN=64, BK=16, exact=True, b_kcontig=True, runv=True, pipe=True),
    "fast_64x64x16_nt": dict(BM=64, BN=64, BK=16, exact=False, b_kcontig=True, pipe=True),
}
KA_ALPHA64 = 72      # alpha, beta as float64 (the f32 kernels' float fields at 56 / 60 are unused here)
KA_BSA64 = 88        # batch stride of A in bytes (u64); B's and C's at 112 / 120 as in the f32 kernels


class Gen64(Gen16x16):
    VT_ALIGN = 2         # (register pairs)

    # ------------------------------------------------------------------ registers
    def alloc_scalars(self):
        S = self.p.salloc
        self.alloc_args()
        self.s_ab = S(4, align=4)                 # alpha (2 registers), beta (2 registers): float64
        self.s_al, self.s_be = self.s_ab.sub(0, 2), self.s_ab.sub(2, 2)
        self.s_a1, self.s_b0 = S(), S()           # 0 when alpha == 1.0 / when beta == +-0.0
        self.s_bsA, self.s_bsBC = S(2, align=2), S(4, align=4)   # batch strides in bytes (grid y = batch index)
        self.s_ldc4, self.s_ldc20 = S(), S()      # here: ldc * 8 bytes, 4 * ldc * 8 (the next accumulator row of a lane)
        self.s_csC4 = None
        self.alloc_pipe()
        self.alloc_sched()

    # ------------------------------------------------------------------ prologue (f32_kernel.Gen.prologue: once, scheduler, run_setup)
    def once(self):
        c, p = self.c, self.p
        e, st = p.emit, self.s_t
        p.note(f"f64 {c.name}: {c.BM}x{c.BN}x{c.BK} tile, 4 waves, wave tile {c.WTM}x{c.WTN}, "
               f"{'laser-order (kc = 256 slices)' if c.exact else 'one accumulation chain'}")
        e("s_load_dwordx8", self.ka0, s(0, 2), KA_A)
        e("s_load_dwordx8", self.ka1, s(0, 2), KA_LDA)
        e("s_load_dwordx4", self.s_ab, s(0, 2), KA_ALPHA64)
        self.batch_offsets(KA_BSA64)
        e("s_xor_b32", st[2], self.s_al[1], 0x3ff00000)
        e("s_or_b32", self.s_a1, st[2], self.s_al[0])
        e("s_and_b32", st[2], self.s_be[1], 0x7fffffff)
        e("s_or_b32", self.s_b0, st[2], self.s_be[0])
        if c.pipe:
            self.pipe_eligible()
        self.lane_setup()

    def pipe_eligible(self):
        """tile transitions of this launch may be pipelined: beta == 0 (the next tile's running sum starts at 0), K a multiple of BK
        (no K-tail masks to undo between tiles), at least three K-tiles (the switch happens two tile bodies before a tile ends)"""
        c, e, st = self.c, self.p.emit, self.s_t
        e("s_and_b32", st[2], self.s_K, c.BK - 1)
        e("s_or_b32", st[2], st[2], self.s_b0)
        e("s_cmp_eq_u32", st[2], 0)
        e("s_cselect_b32", self.s_pipe, 1, 0)
        e("s_cmp_lt_u32", self.s_K, 3 * c.BK)
        e("s_cselect_b32", self.s_pipe, 0, self.s_pipe)

    def kpiece_word(self, pc):
        """A piece (k0 = 2 pc, k0 + 1 of one row): + (pc & 1) * 32 + ((pc >> 1) & 1) * 8 -- chunk 4 * (k / 8) + k % 4 holds k and k + 4"""
        e, t = self.p.emit, self.vt
        e("v_and_b32", t[6], 1, pc)
        e("v_lshl_add_u32", t[5], t[6], 5, t[5])
        e("v_bfe_u32", t[6], pc, 1, 1)
        e("v_lshl_add_u32", t[5], t[6], 3, t[5])

    def xpieces_B(self):
        """B pieces (x-contiguous): x pair px = tid % (BN / 2), row k = tid / (BN / 2) (+ KS per piece, KS = 512 / BN)
        LDS: BM * RS + 2 px * RS + (4 * (k >> 3) + (k & 3)) * 16 + ((k >> 2) & 1) * 8; k = k0 + KS * j with k0 < KS"""
        c, e, t, st = self.c, self.p.emit, self.vt, self.s_t
        RS, tid = c.RS, v(0)
        HB = c.BN // 2
        KS = 256 // HB
        px, k0 = t[0], t[1]
        e("v_and_b32", px, HB - 1, tid)
        e("v_lshrrev_b32", k0, HB.bit_length() - 1, tid)
        e("v_and_b32", t[5], 3, k0)
        e("v_lshlrev_b32", t[5], 4, t[5])                    # (k0 & 3) * 16
        e("v_bfe_u32", t[6], k0, 2, 1)
        e("v_lshl_add_u32", t[5], t[6], 3, t[5])             # + ((k0 >> 2) & 1) * 8      (k0 < 8)
        e("v_mul_u32_u24", t[6], 2 * RS, px)
        e("v_add_u32", t[5], t[5], t[6])
        e("v_add_u32", t[5], c.BM * RS, t[5])
        for j in range(c.NPB):
            kk = KS * j
            cst = 64 * (kk >> 3) + 16 * (kk & 3) + 8 * ((kk >> 2) & 1)
            assert (kk & 3) == 0 or KS >= 8, "k0 and KS * j must not share bits"
            e("v_add_u32", self.WB[j][2], cst, t[5])
            e("v_add_u32", self.WB[j][0], c.STAGE, self.WB[j][2])
            e("v_add_u32", self.WB[j][1], 2 * c.STAGE, self.WB[j][2])
        e("v_mul_lo_u32", t[7], k0, st[5])
        e("v_lshl_add_u32", self.vVB[0], px, 4, t[7])
        e("s_mul_i32", st[4], st[5], KS)
        for j in range(1, c.NPB):
            e("v_add_u32", self.vVB[j], st[4], self.vVB[j - 1])

    def c_row_step(self):
        self.p.emit("s_lshl_b32", self.s_ldc20, self.s_ldc4, 2)

    def b_step(self):
        return self.c.BK * 8 if self.c.b_kcontig else self.s_bstep      # (B passed transposed: a literal)

    # ------------------------------------------------------------------ LDS stores: one ds_write2_b64 per piece
    def store_A_piece(self, pi, ops=None, k=0):
        r = self.stA[pi]
        out = [("vmwait", ("A", pi)),
               ("ldsw", "ds_write2_b64", (self.WA[pi][k], r.sub(0, 2), r.sub(2, 2)), {"offset0": 0, "offset1": 2})]
        if ops is None:
            self.run_ops(out)
        return out

    def store_B_piece(self, pj, ops=None, k=0):
        r = self.stB[pj]
        out = [("vmwait", ("B", pj)),
               ("ldsw", "ds_write2_b64", (self.WB[pj][k], r.sub(0, 2), r.sub(2, 2)),
                {"offset0": 0, "offset1": 2 if self.c.b_kcontig else self.c.RS // 8})]
        if ops is None:
            self.run_ops(out)
        return out

    # ------------------------------------------------------------------ matrix instruction, slice fold
    def emit_mfma(self, b, slot, i, n, u, srcc):
        self.p.emit("v_mfma_f64_16x16x4_f64", self.acc[b], self.fa[slot][i].sub(2 * u, 2), self.fb[slot][n].sub(2 * u, 2), srcc)

    def alpha_mul(self):
        T = self.vT[0]
        return [("v_mul_f64", T.sub(2 * d, 2), self.s_al, T.sub(2 * d, 2)) for d in range(4)]

    def cmp_alpha_one(self):
        self.p.emit("s_cmp_lg_u32", self.s_a1, 0)

    def agpr_add(self, dst):
        e, T = self.p.emit, self.vT[0]
        for d in range(4):
            tt = T.sub(8 + 2 * (d % 2), 2)
            e("v_accvgpr_read_b32", tt[0], dst[2 * d])
            e("v_accvgpr_read_b32", tt[1], dst[2 * d + 1])
            e("v_add_f64", tt, tt, T.sub(2 * d, 2))
            e("v_accvgpr_write_b32", dst[2 * d], tt[0])
            e("v_accvgpr_write_b32", dst[2 * d + 1], tt[1])

    def run_add(self, b):
        if not self.c.runv:
            return self.agpr_add(self.run[b])
        for d in range(4):
            self.p.emit("v_add_f64", self.run[b].sub(2 * d, 2), self.run[b].sub(2 * d, 2), self.vT[0].sub(2 * d, 2))

    # ------------------------------------------------------------------ pipelined tile transitions (f32_kernel.py Cfg.pipe)
    def trans_after(self, b):
        """transition body, block b = (i, n): vT[0..7] hold the slice sum (4 doubles: rows q + 4 d of the block) of the tile being
        FINISHED, the MFMA in front of this gap has restarted the chain for the new tile: C = run + alpha * slice (one chain: alpha *
        sum) leaves for memory from here, the running sum is zeroed for the new tile (beta == 0 in pipelined launches).  Rows (+ 4 d,
        + 16 i) through the stores' scalar offset from srdCd = this wave's first row of the old tile."""
        c, p, e, T, st = self.c, self.p, self.p.emit, self.vT[0], self.s_t
        i, n = b // c.TN, b % c.TN
        assert c.runv or not c.exact
        self.alpha_mul_outlined("t")
        soff = st[0]
        for d in range(4):
            if c.exact:
                tt = T.sub(8 + 2 * (d % 2), 2)
                e("v_add_f64", tt, self.run[b].sub(2 * d, 2), T.sub(2 * d, 2))
                e("v_mov_b64", self.run[b].sub(2 * d, 2), 0)
            else:
                tt = T.sub(2 * d, 2)
            if 16 * i + 4 * d:
                e("s_mul_i32", soff, self.s_ldc4, 16 * i + 4 * d)
            else:
                e("s_mov_b32", soff, 0)
            e("buffer_store_dwordx2", tt, self.vC[n], self.srdCd, soff, offen=True)
            self.vm_issue(("S", b, d))

    def pipe_c_addr(self):
        """(vC, srdCd) for the deferred stores of the tile (m0, n0): srdCd starts at this wave's first row, vC[n] = the lane's offset
        from there (q rows down, block column n; out of bounds beyond N)"""
        r16, q = self.lane_rq()
        self.srdCd_setup()
        self.p.emit("v_mul_lo_u32", self.vt[3], q, self.s_ldc4)
        self.c_columns(r16)

    # ------------------------------------------------------------------ epilogue
    def c_addr_setup(self):
        """vC[n] = byte offset in C of D[q][r16] of block column n: row m0 + wm0 + q (+ 4 per accumulator element, + 16 per
        block row), col n0 + wn0 + r16 + 16n"""
        e, t, st = self.p.emit, self.vt, self.s_t
        r16, q = self.lane_rq()
        e("s_add_u32", st[0], self.s_m0, self.s_wm0)
        e("v_add_u32", t[3], st[0], q)
        e("v_mul_lo_u32", t[3], t[3], self.s_ldc4)
        self.c_columns(r16)

    def c_columns(self, r16):
        """vC[n] = vt[3] (the row's bytes) + the bytes of column n0 + wn0 + r16 + 16 n; out of bounds beyond N"""
        c, e, t, st = self.c, self.p.emit, self.vt, self.s_t
        e("s_add_u32", st[1], self.s_n0, self.s_wn0)
        e("v_add_u32", t[4], st[1], r16)
        e("v_lshl_add_u32", t[3], t[4], 3, t[3])
        for n in range(c.TN):
            e("v_add_u32", t[5], 16 * n, t[4])
            e("v_cmp_gt_u32", VCC, self.s_N, t[5])
            e("v_add_u32", t[6], 128 * n, t[3])
            e("v_mov_b32", t[7], 0x80000000)
            e("v_cndmask_b32", self.vC[n], t[7], t[6], VCC)

    def c_walk(self, fn):
        """visit this lane's accumulator elements in C order: fn(i, d, n) with vC[n] addressing D[q + 4d][r16] of block (i, n)"""
        c = self.c
        for i in range(c.TM):
            for d in range(4):
                fn(i, d)
                if not (i == c.TM - 1 and d == 3):
                    for n in range(c.TN):
                        self.p.emit("v_add_u32", self.vC[n], self.s_ldc20, self.vC[n])

    def load_beta_c(self):
        """laser-order kernels, beta != 0: the running sum starts as beta * C0 (one rounding), loaded through the idle fragment
        registers and drained here, so the loop's counted waits (computed for beta == 0) stay correct"""
        c, p = self.c, self.p
        e = p.emit
        skip = p.label("nobeta")
        e("s_cmp_eq_u32", self.s_b0, 0)
        e("s_cbranch_scc1", skip)
        self.c_addr_setup()
        pool = [r.sub(2 * h, 2) for slot in range(2) for r in (self.fa[slot] + self.fb[slot]) for h in range(2)]
        assert len(pool) >= c.TN

        def row(i, d):
            for n in range(c.TN):
                # (runv: straight into the running sum's own registers)
                dst = self.run[i * c.TN + n].sub(2 * d, 2) if c.runv else pool[n]
                e("buffer_load_dwordx2", dst, self.vC[n], self.srdC, 0, offen=True)
            e("s_waitcnt", vmcnt=0)
            for n in range(c.TN):
                if c.runv:
                    x = self.run[i * c.TN + n].sub(2 * d, 2)
                    e("v_mul_f64", x, self.s_be, x)
                    continue
                e("v_mul_f64", pool[n], self.s_be, pool[n])
                e("v_accvgpr_write_b32", self.run[i * c.TN + n][2 * d], pool[n][0])
                e("v_accvgpr_write_b32", self.run[i * c.TN + n][2 * d + 1], pool[n][1])
        self.c_walk(row)
        p.place(skip)

    def epilogue(self):
        """C = beta * C0 + alpha * (slice sums in order) -- gemm_ukernel_generic.nim:53-76 -- predicated by the descriptor's bounds check"""
        c, p = self.c, self.p
        e = p.emit
        e("s_nop", 15)
        e("s_nop", 7)
        e("s_waitcnt", vmcnt=0, lgkmcnt=0)
        self.vmq.clear()
        self.lgq.clear()
        self.mode_dispatch()
        self.c_addr_setup()
        T = self.vT[0]

        def read_acc(tt, b, d):
            e("v_accvgpr_read_b32", tt[0], self.acc[b][2 * d])
            e("v_accvgpr_read_b32", tt[1], self.acc[b][2 * d + 1])
            e("v_mul_f64", tt, self.s_al, tt)                     # (1.0 * x is x)

        if c.exact:
            def row(i, d):
                for n in range(c.TN):
                    b = i * c.TN + n
                    tt, uu = T.sub(4 * (n % 2), 2), T.sub(4 * (n % 2) + 2, 2)
                    read_acc(tt, b, d)
                    if c.runv:
                        e("v_add_f64", tt, self.run[b].sub(2 * d, 2), tt)
                    else:
                        e("v_accvgpr_read_b32", uu[0], self.run[b][2 * d])
                        e("v_accvgpr_read_b32", uu[1], self.run[b][2 * d + 1])
                        e("v_add_f64", tt, uu, tt)
                    e("buffer_store_dwordx2", tt, self.vC[n], self.srdC, 0, offen=True)
            self.c_walk(row)
        else:
            withc, done = p.label("beta"), p.label("stored")
            e("s_cmp_lg_u32", self.s_b0, 0)
            e("s_cbranch_scc1", withc)

            def row0(i, d):
                for n in range(c.TN):
                    tt = T.sub(4 * (n % 2), 2)
                    read_acc(tt, i * c.TN + n, d)
                    e("buffer_store_dwordx2", tt, self.vC[n], self.srdC, 0, offen=True)
            self.c_walk(row0)
            e("s_branch", done)
            p.place(withc)
            self.c_addr_setup()

            def row1(i, d):
                for n in range(c.TN):
                    e("buffer_load_dwordx2", T.sub(8 + 2 * n, 2), self.vC[n], self.srdC, 0, offen=True)
                e("s_waitcnt", vmcnt=0)
                for n in range(c.TN):
                    tt, x = T.sub(2 * n, 2), T.sub(8 + 2 * n, 2)
                    e("v_mul_f64", x, self.s_be, x)
                    read_acc(tt, i * c.TN + n, d)
                    e("v_add_f64", tt, x, tt)
                    e("buffer_store_dwordx2", tt, self.vC[n], self.srdC, 0, offen=True)
            self.c_walk(row1)
            p.place(done)
        self.end_run()


def make(name, **over):
    kw = dict(CONFIGS[name])
    kw.update(over)
    return Gen64(Cfg(name, dtype="f64", **kw))


if __name__ == "__main__":
    write_kernels("lh_f64_", CONFIGS, make)
