// The channel-group loop of conv_bf16_kernel's bf16 epilogue (included by conv_bf16_tiled.hip inside the kernel body, with MODE in
// scope: 0 = lean order of operations, 1 = general, 2 = both behind a run-time test).  A fragment, not a translation unit.
#pragma unroll
    for (int mb = 0; mb < MW; ++mb) {
#pragma unroll
      for (int gp = 0; gp < 2; ++gp) {
        const int cb = (m0 >> 3) + mb * 4 + 2 * gp;  // channel block the lower half-wave stores (uniform); Mb is even
        if (cb >= p.Mb) continue;
        if constexpr (REF == 1 && RF_PER_GP) {
          const auto rs_r = __builtin_amdgcn_make_buffer_rsrc((void*)(p.act_ref + (size_t)b * p.Mb * plane * 2), (short)0, p.Mb * plane16, RSRC_WORD3);
#pragma unroll
          for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int n = 0; n < NW; ++n) {
              const bool valid = c == 0 ? pvalid[n] : pvalid1[n];
              const int vr = valid ? (opix[n] + c) * 16 + half * 8 + cb * plane16 : (int)0x80000000u;
              rf[0][0][c][n][0] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_r, vr, 0, 0));
              rf[0][0][c][n][1] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_r, vr + plane16, 0, 0));
            }
        }
        const int cl = mb * 32 + 16 * gp + 4 * half;  // local channel of group A; group B = cl + 8
        const float4 bA = *reinterpret_cast<const float4*>(eb + cl), bB = *reinterpret_cast<const float4*>(eb + cl + 8);
        const float4 sA = *reinterpret_cast<const float4*>(es + cl), sB = *reinterpret_cast<const float4*>(es + cl + 8);
        const float ba[8] = {bA.x, bA.y, bA.z, bA.w, bB.x, bB.y, bB.z, bB.w};
        const float sa[8] = {sA.x, sA.y, sA.z, sA.w, sB.x, sB.y, sB.z, sB.w};
        [[maybe_unused]] float s8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, q8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float bs[8], sl[8];  // bias * scale, leaky slope * scale
        [[maybe_unused]] u32x4 stc[NC][NW];   // (stride-2 data gradient: the finished units of both column parities)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          bs[i] = ba[i] * sa[i];
          sl[i] = LEAKY_SLOPE * sa[i];
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
#pragma unroll
          for (int n = 0; n < NW; ++n) {
            // out = act(acc + bias) * scale, or (acc + bias) * act'(ref) * scale.  The channel scale is >= 0 (Dropout2d mask /
            // zero for padding channels), so LeakyReLU commutes with it: one FMA + mul + max per value.
            float v[8];
            if (MODE == 1 || (MODE == 2 && (do_stats || p.act == ACT_SILU || p.out_pre != nullptr || (has_ref && p.ref_act != ACT_LEAKY)))) {  // general order of operations
#pragma unroll
              for (int i = 0; i < 8; ++i) v[i] = acc[c][mb][n][8 * gp + i] + ba[i];
              if (do_stats) {
                if (full_tile) {  // every pixel of the workgroup's tile exists: no masking
#pragma unroll
                  for (int i = 0; i < 8; ++i) {
                    s8[i] += v[i];
                    q8[i] = fmaf(v[i], v[i], q8[i]);
                  }
                } else {
                  const float m = pvalid[n] ? 1.f : 0.f;
#pragma unroll
                  for (int i = 0; i < 8; ++i) {
                    const float vm = v[i] * m;
                    s8[i] += vm;
                    q8[i] = fmaf(vm, v[i], q8[i]);
                  }
                }
              }
              if (p.out_pre != nullptr) {  // the pre-activation goes out through the same 16-byte-unit exchange
                bf16x8 po;   // (bf16_dev.h's pack_unit_swap, open-coded here and below: through the call hipcc orders these epilogues' arithmetic differently)
#pragma unroll
                for (int i = 0; i < 8; ++i) po[i] = (__bf16)v[i];
                const u32x4 pw = __builtin_bit_cast(u32x4, po);
                const auto q0 = __builtin_amdgcn_permlane32_swap(pw.x, pw.z, false, false);
                const auto q1 = __builtin_amdgcn_permlane32_swap(pw.y, pw.w, false, false);
                const u32x4 pst = {q0[0], q1[0], q0[1], q1[1]};
                const auto rs_p = __builtin_amdgcn_make_buffer_rsrc((void*)(p.out_pre + (size_t)b * p.Mb * plane * 2), (short)0, p.Mb * plane16, RSRC_WORD3);
                __builtin_amdgcn_raw_buffer_store_b128(pst, rs_p, vo[c][n] + cb * plane16, 0, 0);
              }
              if constexpr (sign_ref) {  // (the launcher only takes the sign map for LeakyReLU)
                const unsigned m = sg[sign_ref ? c : 0][n][(mb * 2 + gp) >> 2] >> (8 * ((mb * 2 + gp) & 3));
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                  v[i] *= (m >> i) & 1u ? 1.f : LEAKY_SLOPE;
                  v[4 + i] *= (m >> (4 + i)) & 1u ? 1.f : LEAKY_SLOPE;
                }
              } else if (has_ref) {
                const bf16x4 r0 = __builtin_bit_cast(bf16x4, rf[REF == 1 ? mb : 0][RF_PER_GP ? 0 : gp][c][n][0]);
                const bf16x4 r1 = __builtin_bit_cast(bf16x4, rf[REF == 1 ? mb : 0][RF_PER_GP ? 0 : gp][c][n][1]);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                  v[i] *= act_bwd_factor((float)r0[i], p.ref_act);
                  v[4 + i] *= act_bwd_factor((float)r1[i], p.ref_act);
                }
              } else if (p.act == ACT_LEAKY) {  // (uniform branches: a select over all activations would evaluate SiLU's exp)
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = fmaxf(v[i], LEAKY_SLOPE * v[i]);
              } else if (p.act == ACT_SILU) {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = act_fwd(v[i], ACT_SILU);
              }
#pragma unroll
              for (int i = 0; i < 8; ++i) v[i] *= sa[i];
            } else if constexpr (sign_ref) {  // LeakyReLU backward from the sign map (a data gradient: there is no bias)
              const unsigned m = sg[sign_ref ? c : 0][n][(mb * 2 + gp) >> 2] >> (8 * ((mb * 2 + gp) & 3));
#pragma unroll
              for (int i = 0; i < 8; ++i) {
                // bit i spread over a word (v_bfe_i32) selects scale or 0.01 * scale bitwise (v_bfi_b32): three instructions
                // per value with the multiply
                const int t = (int)(m << (31 - i)) >> 31;
#ifndef BF_SIGN_SELECT
                // (v_bfi_b32 by hand: knowing that t is 0 / -1 the optimiser turns the bitwise select into and + compare +
                //  v_cndmask, three instructions where v_bfe_i32 + v_bfi_b32 are two -- these epilogues are bound by vector issue)
                unsigned f;
                asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(f) : "v"(t), "v"(sa[i]), "v"(sl[i]));
#else
                const unsigned f = (__builtin_bit_cast(unsigned, sa[i]) & (unsigned)t) | (__builtin_bit_cast(unsigned, sl[i]) & ~(unsigned)t);
#endif
                v[i] = acc[c][mb][n][8 * gp + i] * __builtin_bit_cast(float, f);
              }
            } else if (has_ref) {  // LeakyReLU backward: factor = ref > 0 ? scale : 0.01 * scale
              const bf16x4 r0 = __builtin_bit_cast(bf16x4, rf[REF == 1 ? mb : 0][RF_PER_GP ? 0 : gp][c][n][0]);
              const bf16x4 r1 = __builtin_bit_cast(bf16x4, rf[REF == 1 ? mb : 0][RF_PER_GP ? 0 : gp][c][n][1]);
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                v[i] = (acc[c][mb][n][8 * gp + i] + ba[i]) * ((float)r0[i] > 0.f ? sa[i] : sl[i]);
                v[4 + i] = (acc[c][mb][n][8 * gp + 4 + i] + ba[4 + i]) * ((float)r1[i] > 0.f ? sa[4 + i] : sl[4 + i]);
              }
            } else {
#pragma unroll
              for (int i = 0; i < 8; ++i) v[i] = fmaf(acc[c][mb][n][8 * gp + i], sa[i], bs[i]);
              if constexpr (MODE == 2) {
                if (p.act == ACT_LEAKY) {
#pragma unroll
                  for (int i = 0; i < 8; ++i) v[i] = fmaxf(v[i], LEAKY_SLOPE * v[i]);
                }
              } else if (leaky) {  // max(v, 0.01 v) as a bare v_max_f32 (fmaxf would first quiet both operands: two more instructions per value)
#pragma unroll
                for (int i = 0; i < 8; i += 2) {
                  const f32x2 sv = (f32x2){v[i], v[i + 1]} * (f32x2){LEAKY_SLOPE, LEAKY_SLOPE};  // one v_pk_mul_f32
                  asm("v_max_f32 %0, %1, %2" : "=v"(v[i]) : "v"(v[i]), "v"(sv.x));
                  asm("v_max_f32 %0, %1, %2" : "=v"(v[i + 1]) : "v"(v[i + 1]), "v"(sv.y));
                }
              }
            }
            if constexpr (SIGN_OUT) if (write_signs) {  // forward of a LeakyReLU block: the sign map the data gradient will read
#ifndef BF_SIGN_CNDMASK
              // byte = sum of (v[i] > 0) << i: the compare leaves its result in vcc and an add-with-carry shifts it into the
              // byte (m = 2 m + carry), values taken from 7 down to 0 -- two vector instructions per value where the compare /
              // select / shift-or form takes three (these tiles are bound by vector-instruction issue)
              // (bf16_dev.h's sign_byte, one statement per value here: hipcc schedules between them)
              unsigned mA = 0;
              constexpr unsigned mB = 0;
#pragma unroll
              for (int i = 7; i >= 0; --i)
                asm("v_cmp_lt_f32_e32 vcc, 0, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc" : "+v"(mA) : "v"(v[i]) : "vcc");
#else
              unsigned mA = 0, mB = 0;
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                mA |= (v[i] > 0.f ? 1u : 0u) << i;
                mB |= (v[4 + i] > 0.f ? 1u : 0u) << i;
              }
#endif
              // one byte = this lane's 4 + 4 signs BEFORE the half-wave exchange of the data below: the data gradient's lanes
              // hold the same channels
              // (the bytes of a pixel collect in a register and go out together behind the group loop: single-byte stores of the
              //  32-channel tiles -- two per pixel group, half-filled 64-byte runs -- cost 0.09 ms of the 16 -> 32 channel forward)
              sg[c][n][(mb * 2 + gp) >> 2] |= (mA | (mB << 4)) << (8 * ((mb * 2 + gp) & 3));
            }
            bf16x8 o;
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = (__bf16)v[i];
            u32x4 w = __builtin_bit_cast(u32x4, o);  // (x, y) = group A, (z, w) = group B of this lane's pixel
            // lanes 32-63 hand their group A down, lanes 0-31 hand their group B up
            const auto r0 = __builtin_amdgcn_permlane32_swap(w.x, w.z, false, false);
            const auto r1 = __builtin_amdgcn_permlane32_swap(w.y, w.w, false, false);
            const u32x4 st = {r0[0], r1[0], r0[1], r1[1]};
            // the channel-block offset goes into the vector offset: with a scalar offset register hipcc (ROCm 7.2) leaves
            // out the wait state between a 16-byte buffer store and a VALU write of its data registers, and gfx950 then
            // stores the overwritten values
            if constexpr (S2D && !BF_S2D_HALF_DENSE) stc[c][n] = st;   // (stored below, both column parities together)
            else __builtin_amdgcn_raw_buffer_store_b128(st, rs_o, vo[c][n] + cb * plane16, 0, BF_ST_AUX);
          }
        }
        if constexpr (S2D && !BF_S2D_HALF_DENSE) {
          // Stride-2 data gradient: a lane's unit of column parity c sits 32 bytes from the next lane's -- stored as they are, the two
          // parities' stores each fill HALF of every 64-byte segment they touch.  A second half-wave exchange (parity 0's upper half-wave =
          // channel block cb + 1 trades places with parity 1's lower half-wave = block cb) makes every store a contiguous kilobyte: lanes
          // 0-31 the even pixel, lanes 32-63 the odd pixel of ONE channel block.  Measured on the direct kernel of layer 2
          // (conv_bf16_direct.hip, gpurun_out/r5_dd_ab*.log): 0.716 -> 0.660 ms with nothing else changed.
#pragma unroll
          for (int n = 0; n < NW; ++n) {
            const auto x0 = __builtin_amdgcn_permlane32_swap(stc[0][n].x, stc[NC - 1][n].x, false, false);
            const auto x1 = __builtin_amdgcn_permlane32_swap(stc[0][n].y, stc[NC - 1][n].y, false, false);
            const auto x2 = __builtin_amdgcn_permlane32_swap(stc[0][n].z, stc[NC - 1][n].z, false, false);
            const auto x3 = __builtin_amdgcn_permlane32_swap(stc[0][n].w, stc[NC - 1][n].w, false, false);
            const u32x4 se0 = {x0[0], x1[0], x2[0], x3[0]}, se1 = {x0[1], x1[1], x2[1], x3[1]};
            __builtin_amdgcn_raw_buffer_store_b128(se0, rs_o, vd[n] + cb * plane16, 0, BF_ST_AUX);
            __builtin_amdgcn_raw_buffer_store_b128(se1, rs_o, vd[n] + (cb + 1) * plane16, 0, BF_ST_AUX);
          }
        }
        if (MODE != 0 && do_stats) {
          // 16 independent DPP chains (the compiler interleaves them), then ONE predicated block of LDS writes
          float sr[8], qr[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            sr[i] = half_wave_sum(s8[i]);
            qr[i] = half_wave_sum(q8[i]);
          }
          if (l31 == 31) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              const int ch = cl + (i < 4 ? i : 4 + i);  // group B starts 8 channels above group A
              red[(wave * BM + ch) * 2 + 0] = sr[i];
              red[(wave * BM + ch) * 2 + 1] = qr[i];
            }
          }
        }
      }
    }
