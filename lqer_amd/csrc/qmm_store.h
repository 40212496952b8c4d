// The store of a finished 128 x 128 tile of the two products (matmul_q.hip), as TEXT: included inside k_qmatmul and k_qmatmul_xr, which
// name the 32 KiB of LDS the 16-bit tile is staged through as QMM_STORE_LDS.  (As a __device__ __forceinline__ function over the
// kernel's accumulators the same statements compile to other code in 12 of the 15 kernels - profiles/attn_pieces_codeobj.txt.)
// Reads the kernel's acc[JT][2], out, b, i0, j0, S1, S2, aligned, tid, wm, wn, l31, lh and its constants T, JT.
// Lane = output row, register r of tile (a, c): column (r & 3) + 8 (r >> 2) + 4 lh.  fp32: stored directly.  16-bit: an accumulator
// quad is packed into 8 B and the quads (2p, 2p + 1) of lanes l / l ^ 32 merged into 16-byte pieces; with the whole tile inside an
// aligned output these go to LDS and leave as full 256-byte row segments (the output is the large stream of Q K^T), else as 16-byte
// stores where the 32 columns lie inside, else as elements.
  const bool staged = DT != LQER_F32 && aligned && j0 + BN <= S2;  // workgroup-uniform
  if (staged) __syncthreads();  // every wave has read its last fragments: the LDS of the tiles is free
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int64_t i = i0 + wm * 64 + c * 32 + l31;
#pragma unroll
    for (int a = 0; a < JT; ++a) {
      const int64_t jb = j0 + wn * (32 * JT) + a * 32;
      if constexpr (DT == LQER_F32) {
        if (i >= S1) continue;
        float* dst = (float*)out + (b * S1 + i) * S2;
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
          const int64_t j = jb + 8 * qd + 4 * lh;
          if (aligned && j + 3 < S2) {
            *(float4*)(dst + j) = make_float4(acc[a][c][4 * qd], acc[a][c][4 * qd + 1], acc[a][c][4 * qd + 2], acc[a][c][4 * qd + 3]);
          } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
              if (j + t < S2) dst[j + t] = acc[a][c][4 * qd + t];
          }
        }
      } else {
        // 16-bit outputs: pack 4 columns into 8 B, then merge quads (2p, 2p+1) of lanes l / l^32 into one 16-byte store
        // (gemm_w4a8.hip's store): lanes 0-31 write columns 16p .. 16p+7, lanes 32-63 columns 16p+8 .. 16p+15 - the output
        // is the large stream of Q K^T (S1 x S2 per head)
        uint32_t pk[4][2];
#pragma unroll
        for (int qd = 0; qd < 4; ++qd)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const float v0 = acc[a][c][4 * qd + 2 * h], v1 = acc[a][c][4 * qd + 2 * h + 1];
            if constexpr (DT == LQER_F16) {
              typedef __attribute__((ext_vector_type(2))) _Float16 h2;
              const h2 hv = {(_Float16)v0, (_Float16)v1};
              pk[qd][h] = __builtin_bit_cast(uint32_t, hv);
            } else {
              pk[qd][h] = (uint32_t)f32_to_bf16_rne(v0) | ((uint32_t)f32_to_bf16_rne(v1) << 16);
            }
          }
        bf16_t* dst = (bf16_t*)out + (b * S1 + i) * S2;
        const bool wide = aligned && jb + 32 <= S2;  // wave-uniform
        if (staged) {
          // whole tile inside the output: the 16-byte pieces go to LDS (row-major 256 B per row, chunks XOR-ed with the row
          // so that the 32 rows of a wave's store spread over the banks) and leave as full 256-byte row segments below
          const int row_l = wm * 64 + c * 32 + l31;
#pragma unroll
          for (int p2 = 0; p2 < 2; ++p2) {
            auto r0 = __builtin_amdgcn_permlane32_swap(pk[2 * p2][0], pk[2 * p2 + 1][0], false, false);
            auto r1 = __builtin_amdgcn_permlane32_swap(pk[2 * p2][1], pk[2 * p2 + 1][1], false, false);
            const int chunk = (wn * (32 * JT) + a * 32 + 16 * p2 + 8 * lh) >> 3;
            *(uint4*)(QMM_STORE_LDS + row_l * 256 + ((chunk ^ (row_l & 15)) << 4)) = make_uint4(r0[0], r1[0], r0[1], r1[1]);
          }
        } else if (wide) {
#pragma unroll
          for (int p2 = 0; p2 < 2; ++p2) {
            auto r0 = __builtin_amdgcn_permlane32_swap(pk[2 * p2][0], pk[2 * p2 + 1][0], false, false);
            auto r1 = __builtin_amdgcn_permlane32_swap(pk[2 * p2][1], pk[2 * p2 + 1][1], false, false);
            if (i < S1) *(uint4*)(dst + jb + 16 * p2 + 8 * lh) = make_uint4(r0[0], r1[0], r0[1], r1[1]);
          }
        } else if (i < S1) {
#pragma unroll
          for (int qd = 0; qd < 4; ++qd) {
            const int64_t j = jb + 8 * qd + 4 * lh;
            if (j < S2) dst[j] = (bf16_t)(pk[qd][0] & 0xffff);
            if (j + 1 < S2) dst[j + 1] = (bf16_t)(pk[qd][0] >> 16);
            if (j + 2 < S2) dst[j + 2] = (bf16_t)(pk[qd][1] & 0xffff);
            if (j + 3 < S2) dst[j + 3] = (bf16_t)(pk[qd][1] >> 16);
          }
        }
      }
    }
  }
  if (staged) {
    __syncthreads();
    bf16_t* const ob = (bf16_t*)out + (b * S1) * S2 + j0;
#pragma unroll
    for (int u = 0; u < 2048 / T; ++u) {  // 16 consecutive lanes = one row of the tile: 256 contiguous bytes
      const int idx = tid + T * u, row_l = idx >> 4, chunk = idx & 15;
      const uint4 v = *(const uint4*)(QMM_STORE_LDS + row_l * 256 + ((chunk ^ (row_l & 15)) << 4));
      if (i0 + row_l < S1) *(uint4*)(ob + (i0 + row_l) * S2 + chunk * 8) = v;
    }
  }
