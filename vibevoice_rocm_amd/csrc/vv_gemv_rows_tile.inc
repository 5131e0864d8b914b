// vv_gemv_rows_tile.inc - the activation prologue's lay-out of ONE row tile (rows 8 t .. 8 t + 7: `constexpr int t` is the includer's), included
// once per tile by vv_gemv_rows_body.inc: normalise, modulate, split into bf16 hi / lo and store in fragment order.  Text, not a loop over t: a
// loop (of one trip) in front of the 8-row kernels changes their register allocation.
      unsigned char* base = smem + ((size_t)((wv * KA + j) * 64 + cq * 16) * 16 + half * 8);
      if constexpr (RT > 1) base += (size_t)t * (NW * KA * 64 * 16);
      if constexpr (MOD_OK && RT > 1) {
        if (t > 0 && has_mod) {                        // the next tile's adaLN rows
#pragma unroll
          for (int m = 0; m < 8; ++m) {
            const int64_t mo = (int64_t)(8 * t + m < mr ? 8 * t + m : mr - 1) * a.ld_mod + k0 + 4 * q;
            sv[m][cc] = *reinterpret_cast<const float4*>(a.mod_shift + (cval[cc] ? mo : 0));
            cv[m][cc] = *reinterpret_cast<const float4*>(a.mod_scale + (cval[cc] ? mo : 0));
          }
        }
      }
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        float4 v = xv[8 * t + m][cc];
        if (rms) {
          const float r = rstd[8 * t + m];
          v.x *= r; v.y *= r; v.z *= r; v.w *= r;
          if (has_nw) { v.x *= nv[cc].x; v.y *= nv[cc].y; v.z *= nv[cc].z; v.w *= nv[cc].w; }
          if constexpr (MOD_OK) {
            if (has_mod) {
              v.x = v.x * (1.0f + cv[m][cc].x) + sv[m][cc].x; v.y = v.y * (1.0f + cv[m][cc].y) + sv[m][cc].y;
              v.z = v.z * (1.0f + cv[m][cc].z) + sv[m][cc].z; v.w = v.w * (1.0f + cv[m][cc].w) + sv[m][cc].w;
            }
          }
        }
        if (!cval[cc] || 8 * t + m >= mr) v = make_float4(0.f, 0.f, 0.f, 0.f);
        const unsigned h0 = bf16_bits(v.x), h1 = bf16_bits(v.y), h2 = bf16_bits(v.z), h3 = bf16_bits(v.w);
        const float l0 = v.x - __uint_as_float(h0 << 16), l1 = v.y - __uint_as_float(h1 << 16);
        const float l2 = v.z - __uint_as_float(h2 << 16), l3 = v.w - __uint_as_float(h3 << 16);
        u32x2 hi, lo;
        hi.x = h0 | (h1 << 16); hi.y = h2 | (h3 << 16);
        lo.x = bf16_bits(l0) | (bf16_bits(l1) << 16); lo.y = bf16_bits(l2) | (bf16_bits(l3) << 16);
        *reinterpret_cast<u32x2*>(base + (size_t)m * 16) = hi;               // fragment row m: high parts
        *reinterpret_cast<u32x2*>(base + (size_t)(m + 8) * 16) = lo;         // fragment row m + 8: low parts
      }
