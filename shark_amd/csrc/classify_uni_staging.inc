// classify_uni_staging.inc -- a fragment of classify_uni_kernel's BODY (classify_uni.hpp includes it where it stands; not a header of its own):
// staging: a read's bases -> two streams of 2-bit codes + validity bits in the wave's LDS area (16 bases per lane for three pairs, 8 per lane otherwise).
    // ---- stage: 8 bases per lane -> the two code streams + validity (see process_read) ----
    uint32_t inv_real = 0u;   // invalid characters among the lane's bases that belong to the read
    // (stage_bases.hpp: without multiplies where the table lies in LDS -- instruction-bound, 128 VGPRs to their name; the instantiations
    //  that probe tables in memory are held at 80 VGPRs, spill a few as it is, and keep the form they had)
    constexpr bool STG_MUL = SHK_STAGE_MUL || !UG::LX;
    if (TRI) {
      // sixteen bases of pair tri_pr of the triple into that pair's area: the same three streams, a dword / a dword / 16 bits per chunk
      if (tri_act && 3u * it + tri_pr < n_reads) {
        const uint32_t sh = t_cur.sh;
        const uint32_t b0 = __builtin_amdgcn_alignbyte(t_cur.d1, t_cur.d0, sh), b1 = __builtin_amdgcn_alignbyte(t_cur.d2, t_cur.d1, sh);
        const uint32_t b2 = __builtin_amdgcn_alignbyte(t_cur.d3, t_cur.d2, sh), b3 = __builtin_amdgcn_alignbyte(t_cur.d4, t_cur.d3, sh);
        uint32_t msb32, inv16;      // first base in bits 31:30, in bit 0
        stage16(b0, b1, b2, b3, msb32, inv16);
        uint32_t tail16 = tri_tail;
        if (TRO && !(SHK_TRO_ABL & 4)) {   // what lies behind the read's own end is invalid (the layout is the longest mates')
          const uint32_t rem = tlr_cur > tri_bofs ? tlr_cur - tri_bofs : 0u;
          tail16 = rem < 16u ? (0xFFFFu << rem) & 0xFFFFu : 0u;
        }
        inv16 |= tail16;
        const uint32_t lsb32 = stg_lsb_first(msb32);
        uint64_t *area = wbase + tri_pr * WORDS;
        uint32_t *fwa = reinterpret_cast<uint32_t *>(area);
        fwa[tri_cl] = lsb32;
        (fwa + code_dwords_for(S))[(rcap >> 4) - 1u - tri_cl] = msb32;
        reinterpret_cast<uint16_t *>(area + code_dwords_for(S))[tri_cl] = (uint16_t)(~inv16 & 0xFFFFu);
        inv_real = inv16 & ~tail16;   // (TRO: a short mate is not an invalid character -- its pair's slots end where it ends: nk1e / nk2e below)
      }
    }
#pragma unroll
    for (int g = 0; g < (TRI ? 0 : G); ++g) {
      if (act[g]) {
        const uint32_t gi = (uint32_t)lane + 64u * g;
        const uint32_t sh = w_cur[g].shn & 3u;
        const uint32_t lo = __builtin_amdgcn_alignbyte(w_cur[g].d1, w_cur[g].d0, sh);
        const uint32_t hi = __builtin_amdgcn_alignbyte(w_cur[g].d2, w_cur[g].d1, sh);
        uint32_t msb16, inv8;                                              // first base in bits 15:14, in bit 0
        stage8<STG_MUL>(lo, hi, msb16, inv8);
        // (bytes behind the mate's end are whatever follows in the buffer: their codes land at packed positions that no
        // existing slot's window covers, and tail_inv marks them invalid)
        inv8 |= tail_inv[g];
        if (HASQ) {
          const uint32_t qs = q_cur[g].shn & 3u;
          const uint32_t qlo = __builtin_amdgcn_alignbyte(q_cur[g].d1, q_cur[g].d0, qs);
          const uint32_t qhi = __builtin_amdgcn_alignbyte(q_cur[g].d2, q_cur[g].d1, qs);
          inv8 |= gather8<STG_MUL>(qmask4(qlo, P.mq), qmask4(qhi, P.mq));
        }
        const uint32_t lsb = stg_lsb_first(msb16);                         // lands in the high half
        reinterpret_cast<uint16_t *>(fw)[gi] = (uint16_t)(lsb >> 16);
        reinterpret_cast<uint16_t *>(rv)[(rcap >> 3) - 1u - gi] = (uint16_t)msb16;
        reinterpret_cast<uint8_t *>(vbits)[gi] = (uint8_t)(~inv8 & 0xFFu);
        inv_real |= inv8 & ~tail_inv[g];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    SHK_STAMP(1);
#if SHK_STAMPS
    if constexpr (TRI) st_acc[8] += 1;
#endif
