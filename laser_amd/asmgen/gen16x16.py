"""What the two families built on 16x16-block matrix instructions share (f64_kernel.Gen64: v_mfma_f64_16x16x4_f64, f32x16_kernel.Gen16:
v_mfma_f32_16x16x4_f32): the program structure is f32_kernel.Gen's, the LDS image and the lane maps are their own.

LDS image (per stage: A panel rows 0..BM-1, then the B panel rows = columns of the tile): a row holds 128 bytes of k as 8 chunks of 16
bytes plus 16 bytes of padding -- 144 bytes, 9 chunks: the 16 rows a 16-lane group reads fall into 16 different 4-bank groups, so the
ds_read_b128 fragment reads are conflict-free without a swizzle.  Which k a chunk holds is the family's (kpiece_word, xpieces_B).
Pieces of a k-contiguous operand: piece column pc = tid % 8, row xr = tid / 8 (+ 32 per piece).  Lane l of a wave feeds A[l % 16][l / 16]
and B[l / 16][l % 16] (r16 = l % 16, q = l / 16).  Each family states its registers (alloc_scalars), its stores to LDS
(store_A_piece / store_B_piece), its arithmetic on a block (emit_mfma and the slice-fold hooks of f32_kernel.Gen) and its epilogue."""
from .core import v
from .f32_kernel import Gen


class Gen16x16(Gen):
    VT_ALIGN = 4         # alignment of the slice-sum temporaries vT

    # ------------------------------------------------------------------ registers
    def alloc(self):
        c, p = self.c, self.p
        S, V = p.salloc, p.valloc
        # (the debug dumps of f32_kernel.Gen name its own address-register layout)
        assert c.BM % 32 == 0 and c.BN % 32 == 0 and c.BK * c.ESZ == 128 and not c.debug and not c.deep
        self.alloc_scalars()
        self.acc = [p.aalloc(c.ACCR) for _ in range(c.NB)]
        # runv (f32_kernel.py Cfg): the running sum in arch VGPRs -- the slice fold adds to it in place, where the all-AGPR plan moves
        # every register out and back; dataa: fragments + staging in AGPRs (the tiles whose VGPR file would overflow)
        self.run = [V(c.ACCR) if c.runv else p.aalloc(c.ACCR) for _ in range(c.NB)] if c.exact else None
        D4 = (lambda n: p.aalloc(n)) if c.dataa else V
        self.fa = [[D4(4) for _ in range(c.TM)] for _ in range(2)]
        self.fb = [[D4(4) for _ in range(c.TN)] for _ in range(2)]
        self.stA = [D4(4) for _ in range(c.NPA)]
        self.stB = [D4(4) for _ in range(c.NPB)]
        self.st_sets = [(self.stA, self.stB)]
        self.RA = [[V() for _ in range(3)] for _ in range(c.NG)]
        self.RB = [[V() for _ in range(3)] for _ in range(c.NG)]
        self.WA = [[V() for _ in range(3)] for _ in range(c.NPA)]   # [piece][stage]
        self.WB = [[V() for _ in range(3)] for _ in range(c.NPB)]
        self.v_oob = V()
        self.s_tm = S(2)
        self.s_ktail = S()
        self.s_em = []              # (16-byte pieces are all-or-nothing: K is a multiple of their elements)
        self.vVA = [V() for _ in range(c.NPA)]
        self.vVB = [V() for _ in range(c.NPB)]
        self.vC = [V() for _ in range(c.TN)]
        self.ndump = 0
        self.dump_names = []
        self.vT = [V(16, align=self.VT_ALIGN)]
        blk = V(12, align=4)
        self.vt = [blk[i] for i in range(10)]
        self.vF, self.vFaddr, self.vFoff = blk.sub(4, 4), blk[10], blk[11]

    # ------------------------------------------------------------------ prologue (f32_kernel.Gen.prologue: once, scheduler, run_setup)
    def lane_rq(self):
        """(r16, q) of this lane, in vt[1], vt[2]"""
        e, t = self.p.emit, self.vt
        e("v_and_b32", t[0], 63, v(0))
        e("v_and_b32", t[1], 15, t[0])
        e("v_lshrrev_b32", t[2], 4, t[0])
        return t[1], t[2]

    def lane_setup(self):
        """the part of once() behind the kernel arguments: wave tile origin, the LDS addresses of the fragment reads and of the pieces'
        stores, B's global offsets and its step per K-tile"""
        c, p = self.c, self.p
        e = p.emit
        t, st = self.vt, self.s_t
        RS = c.RS
        tid = v(0)
        lane, r16, q = t[0], t[1], t[2]
        e("v_and_b32", lane, 63, tid)
        e("v_lshrrev_b32", t[5], 6, tid)
        e("s_nop", 1, comment="VALU write -> v_readfirstlane of the same VGPR needs wait states")
        e("v_readfirstlane_b32", self.s_wave, t[5])
        e("s_nop", 3)
        e("v_and_b32", r16, 15, lane)
        e("v_lshrrev_b32", q, 4, lane)
        e("s_lshr_b32", st[2], self.s_wave, 1)
        e("s_mul_i32", self.s_wm0, st[2], c.WTM)
        e("s_and_b32", st[2], self.s_wave, 1)
        e("s_mul_i32", self.s_wn0, st[2], c.WTN)
        # fragment reads of group g: (wm0 + r16) * RS [+ BM * RS + (wn0 + r16) * RS for B] + (4g + q) * 16
        e("v_add_u32", t[5], self.s_wm0, r16)
        e("v_mul_u32_u24", t[6], RS, t[5])
        e("v_add_u32", t[5], self.s_wn0, r16)
        e("v_mul_u32_u24", t[7], RS, t[5])
        e("v_add_u32", t[7], c.BM * RS, t[7])
        for g in range(c.NG):
            e("v_lshl_add_u32", t[5], q, 4, 64 * g)
            for R, row in ((self.RA, t[6]), (self.RB, t[7])):
                e("v_add_u32", R[g][0], t[5], row)
                e("v_add_u32", R[g][1], c.STAGE, R[g][0])
                e("v_add_u32", R[g][2], 2 * c.STAGE, R[g][0])
        pc, xr = t[0], t[1]
        e("v_and_b32", pc, 7, tid)
        e("v_lshrrev_b32", xr, 3, tid)
        e("v_mov_b32", self.v_oob, 0x80000000)
        # k-contiguous pieces (A always; B when it is passed transposed):  LDS: row * RS + (pc >> 2) * 64 + the family's kpiece_word
        e("v_lshrrev_b32", t[5], 2, pc)
        e("v_lshlrev_b32", t[5], 6, t[5])
        self.kpiece_word(pc)
        e("v_mul_u32_u24", t[6], RS, xr)
        e("v_add_u32", t[5], t[5], t[6])
        for i in range(c.NPA):
            e("v_add_u32", self.WA[i][2], 32 * RS * i, t[5])
            e("v_add_u32", self.WA[i][0], c.STAGE, self.WA[i][2])
            e("v_add_u32", self.WA[i][1], 2 * c.STAGE, self.WA[i][2])
        e("s_lshl_b32", st[5], self.s_ldb, c.ESZ.bit_length() - 1, comment=f"ldb * {c.ESZ} bytes")
        if c.b_kcontig:
            # B passed transposed: its pieces are (column x, k0 ..) -- the A layout with the B panel's offsets
            e("v_add_u32", t[5], c.BM * RS, t[5])
            for j in range(c.NPB):
                e("v_add_u32", self.WB[j][2], 32 * RS * j, t[5])
                e("v_add_u32", self.WB[j][0], c.STAGE, self.WB[j][2])
                e("v_add_u32", self.WB[j][1], 2 * c.STAGE, self.WB[j][2])
            e("s_mov_b32", self.s_bstep, c.BK * c.ESZ)
        else:
            self.xpieces_B()
            e("s_mul_i32", self.s_bstep, st[5], c.BK, comment="B advances BK rows per K-tile")

    def kcontig_goff(self, Voff, NP, ld_bytes):
        """global offsets of a k-contiguous operand's pieces: (xr + 32 i) * ld bytes + pc * 16, pc = tid % 8, xr = tid / 8 (per run: the K
        tail of a run overwrites them with the out-of-bounds offset)"""
        e, t, st = self.p.emit, self.vt, self.s_t
        e("v_and_b32", t[0], 7, v(0))
        e("v_lshrrev_b32", t[1], 3, v(0))
        e("v_mul_lo_u32", t[7], t[1], ld_bytes)
        e("v_lshl_add_u32", Voff[0], t[0], 4, t[7])
        e("s_lshl_b32", st[4], ld_bytes, 5)                  # 32 rows
        for i in range(1, NP):
            e("v_add_u32", Voff[i], st[4], Voff[i - 1])

    def mask_last_pieces_if(self, sreg, value):
        pass      # (no piece straddles K)

    def zero_run(self):
        if not self.c.runv:
            return super().zero_run()
        for b in range(self.c.NB):
            for j in range(self.c.ACCR // 2):
                self.p.emit("v_mov_b64", self.run[b].sub(2 * j, 2), 0)

    # ------------------------------------------------------------------ LDS stores: the family's store_A_piece / store_B_piece
    def staging_ops(self, wr_k):
        c, stg = self.c, []
        for pi in range(c.NPA):
            stg += self.store_A_piece(pi, ops=[], k=wr_k)
            stg.append(("loadA", pi))
        for pj in range(c.NPB):
            stg += self.store_B_piece(pj, ops=[], k=wr_k)
            stg.append(("loadB", pj))
        return stg
