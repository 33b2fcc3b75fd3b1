// ph_kernels_fused_multi_body.h - the body of ph_kernels_fused_multi.hip's kernels, included once per kernel: the single frame's
// (PH_FM_BATCH 0; `a`: its FusedMultiArgs) and the batched launch's (PH_FM_BATCH 1; `a`: what the jobs share, FusedMultiBatchArgs::m).
// One text, so the two cannot drift apart - and the single frame's kernel is compiled from the tokens it always had: a body shared
// through a function, even an inlined one, reaches the scheduler as other IR and comes out in another instruction order.
// A batched launch is gridDim.y frames side by side: the workgroups (x, j), x = 0..gridDim.x - 1 - in the order workgroups are numbered,
// [j * gridDim.x, (j + 1) * gridDim.x) - own job j and divide ITS quads among them as the workgroups of a single frame do.  The job is
// uniform per workgroup: its layer and plane pointers are scalar loads from the argument block at an offset made from blockIdx.y.
// Everything else - geometry, the reader recipe, the output descriptors but for their planes - is the launch's.
// PH_FM_TRANS 1 (ph_kernels_fused_trans.hip; `a`: FusedTransArgs::m): the single frame's kernel with layers that may be in a dissolve or a
// wipe - such a layer leaves the rolled loop's plain path for fm_trans_layer; everything else, phase 2 included, is the text below.
// PH_FM_ROUTE 1 (ph_kernels_fused_route.hip; `a`: FusedRouteArgs::m; IMG: the launch has an image layer): the single frame's kernel with
// layers that may be f32 RGBA images - such a layer leaves the plain path for fm_route_image_layer - and the combined image as an output
// (karg->image_out, stored at the end of phase 1).  There the combine is ph_combine's to the bit: the bottom layer is assigned, and with
// IMG the six alphas are carried.  n_out may be 0: no phase 2.
// PH_FM_FIELD 1 (ph_kernels_fused_field.hip; `a`: FusedFieldArgs::m or FusedFieldBatchArgs::b.m - both begin with the whole-frame kernel's
// arguments, which is what the kernarg pointers below are cast to; first_line: the kernel's own): the outputs all take the same field and
// only its lines are composed.  a.total_quads, the ranges, the tiles, the wave skipping and the tail lanes are the field's; a field quad's
// place in the frame (ph_fused_field.h) is made where a slice loads (quad_of) and where it stores (phase 2).
#if PH_FM_ROUTE
  constexpr int P = PH_FM_ROUTE_P, BS = kLdsBlock;
#else
  constexpr int P = 6, BS = kLdsBlock;
#endif
#if PH_FM_TRANS || PH_FM_ROUTE
#define PH_FM_LUT_LOAD(v) fm_lut_load<BS>(v)  // (lds_lut_load with the lane's place made at the load: ph_kernels_fused_out.h)
#else
#define PH_FM_LUT_LOAD(v) lds_lut_load<BS>(v)
#endif
  // The output descriptors are walked by run-time index (table groups, the outputs of a group).  Read through the argument struct
  // that would put a private copy of all of it in scratch; read where they are - the explicit arguments lie at the start of the
  // kernel-argument segment - they stay scalar loads at a computed offset.
#if PH_FM_TRANS
  typedef const __attribute__((address_space(4))) FusedTransArgs *fm_kernarg_ptr;
  const auto *const karg = (fm_kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
  const auto *const outs = karg->m.out;
#elif PH_FM_ROUTE
  typedef const __attribute__((address_space(4))) FusedRouteArgs *fm_kernarg_ptr;
  const auto *const karg = (fm_kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
  const auto *const outs = karg->m.out;
#elif PH_FM_BATCH
  typedef const __attribute__((address_space(4))) FusedMultiBatchArgs *fm_kernarg_ptr;
  const auto *const karg = (fm_kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
  const auto *const outs = karg->m.out;
#else
  typedef const __attribute__((address_space(4))) FusedMultiArgs *fm_kernarg_ptr;
  const auto *const outs = ((fm_kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr())->out;
#endif
  const ReadK rk = load_read_k(a.rd_cm, a.rd_gm);
  const LutK rlut = make_lut_k(a.rd);
  const bool std_matrix = ycbcr_matrix_is_standard(rk);  // uniform
#if PH_FM_TRANS || PH_FM_ROUTE
  auto layer_ptr = [&](int l) { return reinterpret_cast<const uint4 *>(karg->m.layers[l]); };
#elif PH_FM_BATCH
  auto layer_ptr = [&](int l) { return reinterpret_cast<const uint4 *>(karg->layers[blockIdx.y][l]); };
#else
  auto layer_ptr = [&](int l) { return reinterpret_cast<const uint4 *>(a.layers[l]); };
#endif
  // every workgroup owns one contiguous, equally sized range of quads - it begins and ends wherever that falls, in mid-line too -
  // and walks it in tiles of BS * P quads; only the last tile of a range is partially filled
  const uint32_t per_wg = (a.total_quads + gridDim.x - 1) / gridDim.x;
  const uint32_t wg_begin = blockIdx.x * per_wg;
  const uint32_t wg_end = wg_begin + per_wg < a.total_quads ? wg_begin + per_wg : a.total_quads;
  const uint32_t tile_quads = BS * P;
  for (uint32_t tile_begin = wg_begin; tile_begin < wg_end; tile_begin += tile_quads) {
    uint32_t st[P][9];
    // (pinned per tile, like the reader table's place below: what the lanes derive from them is made in the tile, not kept in
    // registers through it for a next tile that a frame-sized share does not have)
    uint32_t last_quad = wg_end - 1;
    asm volatile("" : "+s"(last_quad));
#if PH_FM_FIELD
    // the range, the tile and the tail are the FIELD's; what a slice loads at is that quad's place in the frame, made where the slice
    // asks for it from a pinned copy of the lane (left alone, all six slices' are made in front of the loop and kept through it)
    auto quad_of = [&](int p) {
      uint32_t lane = threadIdx.x;
      asm volatile("" : "+v"(lane));
      const uint32_t g = tile_begin + p * BS + lane;
      return fused_field_quad(g < wg_end ? g : last_quad, a.quads_per_line, a.magic_qpl, first_line).f;
    };
#else
    auto quad_of = [&](int p) {
      const uint32_t f = tile_begin + p * BS + threadIdx.x;  // width % 48 == 0: flat index == offset
      return f < wg_end ? f : last_quad;                      // tail lanes recompute the last quad
    };
#endif
    // one-deep prefetch through layers and slices; the very first word is requested before the table load
#if PH_FM_ROUTE
    // (an image layer's slot in the chain stays empty: its v210 word is not loaded, its texels are fm_route_image_layer's)
    auto is_image = [&](int l) { return IMG && karg->is_image[l] != 0; };  // uniform
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (!is_image(0)) w = load_stream(layer_ptr(0) + quad_of(0));
    bool own = false;  // the lane's quad of the slice is its own, not a tail lane's copy of the last one: set per slice
#else
    uint4 w = load_stream(layer_ptr(0) + quad_of(0));
#endif
    auto phase1_slice = [&](auto tag, uint4 w, uint32_t f, uint32_t f_next, bool more, uint32_t(&st)[9]) -> uint4 {
      float acc[18];
#pragma unroll
      for (int i = 0; i < 18; ++i) acc[i] = 0.0f;
#if PH_FM_ROUTE
      float al[IMG ? 6 : 1];  // the six alphas: carried only where a layer's can differ from 1
#pragma unroll
      for (int j = 0; j < (IMG ? 6 : 1); ++j) al[j] = 1.0f;
#endif
#pragma unroll 1  // rolled: one copy of the per-layer code whatever N is
      for (int l = 0; l < N; ++l) {
        uint4 nxt = w;
#if PH_FM_ROUTE
        if (l + 1 < N) {
          if (!is_image(l + 1)) nxt = load_stream(layer_ptr(l + 1) + f);
        } else if (more) {
          if (!is_image(0)) nxt = load_stream(layer_ptr(0) + f_next);
        }
        if (is_image(l)) {
          fm_route_image_layer(acc, al, karg->m.layers[l], l, f);
          w = nxt;
          continue;
        }
#else
        if (l + 1 < N) nxt = load_stream(layer_ptr(l + 1) + f);
        else if (more) nxt = load_stream(layer_ptr(0) + f_next);
#endif
#if PH_FM_TRANS
        if (karg->kind[l] != kFusedCut) {  // uniform: the layer is in a transition
          fm_trans_layer<decltype(tag)::value>(acc, w, karg, l, f, rk, rlut);
          w = nxt;
          continue;
        }
#endif
        const Yuv6 q = unpack_quad(w);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          const float4 t = read_px_lds<decltype(tag)::value>(q.y[j], q.cb[j >> 1], q.cr[j >> 1], rk, rlut, 1.0f);
          const float kk = 1.0f - t.w;
#if PH_FM_ROUTE
          if (l == 0) {  // uniform: the bottom layer is taken as it is, its -0 included (ph_combine)
            acc[3 * j] = t.x, acc[3 * j + 1] = t.y, acc[3 * j + 2] = t.z;
            continue;
          }
          if (IMG) al[j] = fma_rn(al[j], 0.0f, t.w);  // NaN above an image pixel whose alpha is Inf or NaN
#endif
          // acc = fma(acc, kk, t), acc as destination (combine.ts:45-65; layer 0: fma(0, k, t) == t)
          asm volatile("v_fma_f32 %0, %0, %3, %4\n\tv_fma_f32 %1, %1, %3, %5\n\tv_fma_f32 %2, %2, %3, %6"
                       : "+v"(acc[3 * j]), "+v"(acc[3 * j + 1]), "+v"(acc[3 * j + 2])
                       : "v"(kk), "v"(t.x), "v"(t.y), "v"(t.z));
        }
        w = nxt;
      }
#if PH_FM_ROUTE
      if (karg->image_out && own) {  // the combined image, as ph_combine stores it (without an image layer its alpha is the chain's fma(1, 0, 1))
        float4 *const po = reinterpret_cast<float4 *>(karg->image_out) + (size_t)f * 6u;
#pragma unroll
        for (int j = 0; j < 6; ++j) store_image(po + j, make_float4(acc[3 * j], acc[3 * j + 1], acc[3 * j + 2], al[IMG ? j : 0]), karg->nt);
      }
      if (a.n_out)  // uniform
#endif
#pragma unroll
      for (int i = 0; i < 9; ++i) {  // the writers' first step needs no table: the 16-bit indices, two per register
        const uint32_t lo = __float_as_uint(lds_lut_index_unit(acc[2 * i]));
        const uint32_t hi = __float_as_uint(lds_lut_index_unit(acc[2 * i + 1]));
        st[i] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
        asm volatile("" : "+v"(st[i]));  // pinned: keeps phase 1's arithmetic in front of the barrier
      }
      return w;
    };
    {
      LutView rd = a.rd;
      asm volatile("" : "+s"(rd.blob), "+s"(rd.hole));
      PH_FM_LUT_LOAD(rd);
    }
    __syncthreads();
    // a slice is skipped per WAVE: only the waves that hold quads of a partly filled slice run it
    const uint32_t wave_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u));
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const uint32_t f = quad_of(p);
      if (p * BS + wave_first < wg_end - tile_begin) {
        PH_FM_BALANCE(p);
        const bool more = (p + 1 < P) && ((p + 1) * BS + wave_first < wg_end - tile_begin);
        const uint32_t f_next = more ? quad_of(p + 1) : f;
#if PH_FM_ROUTE
        own = tile_begin + p * BS + threadIdx.x < wg_end;
#endif
        if (std_matrix) w = phase1_slice(std::true_type{}, w, f, f_next, more, st[p]);
        else w = phase1_slice(std::false_type{}, w, f, f_next, more, st[p]);
      }
    }
    // phase 2, once per distinct writer table (the outputs arrive grouped by table)
#pragma unroll 1
    for (uint32_t k0 = 0; k0 < a.n_out;) {
      const LutView wr{outs[k0].wr.blob, outs[k0].wr.bytes, outs[k0].wr.hole, outs[k0].wr.bias, outs[k0].wr.shift, outs[k0].wr.a_scale, outs[k0].wr.delta_scale, outs[k0].wr.delta_base};
      uint32_t k1 = k0 + 1;
      while (k1 < a.n_out && outs[k1].wr.blob == wr.blob) ++k1;  // uniform
      __syncthreads();  // nobody reads the table in the LDS any more
      PH_FM_LUT_LOAD(wr);
      __syncthreads();
      const LutK wlut = make_lut_k(wr);
      uint32_t lane_quad = tile_begin + threadIdx.x;
      asm volatile("" : "+v"(lane_quad));  // (pinned: every slice's quad, line and column are made here, not kept from in front of the loop)
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const uint32_t f = lane_quad + p * BS;
        if (p * BS + wave_first < wg_end - tile_begin) {
          PH_FM_BALANCE(p);
          float g[18];
#pragma unroll
          for (int i = 0; i < 9; ++i) {  // M + idx: the index ORed into the mantissa of 1.5 * 2^23
            // (pinned: the expansion does not depend on the table, and left alone all 108 expanded indices of the tile are made
            // in front of the loop over the tables and kept through it - twice the registers the packed ones take)
            asm volatile("" : "+v"(st[p][i]));
            g[2 * i] = lds_lut_fetch(wlut, __uint_as_float((st[p][i] & 0xFFFFu) | 0x4B400000u));
            g[2 * i + 1] = lds_lut_fetch(wlut, __uint_as_float((st[p][i] >> 16) | 0x4B400000u));
            // two pixels' twelve LDS reads in flight at a time: all thirty-six at once would want registers this kernel does not have
            if (i % 3 == 2) __builtin_amdgcn_sched_barrier(0);
          }
#if PH_FM_FIELD
          if (f < wg_end) {  // (f: the FIELD quad; the outputs' takes are 0 - every line composed is theirs)
            const FieldQuad at = fused_field_quad(f, a.quads_per_line, a.magic_qpl, first_line);
#pragma unroll 1
#if PH_FM_BATCH
            for (uint32_t k = k0; k < k1; ++k) fused_out_store(outs[k], karg->plane[blockIdx.y][k], g, at.f, at.line, at.col);
#else
            for (uint32_t k = k0; k < k1; ++k) fused_out_store(outs[k], outs[k].plane, g, at.f, at.line, at.col);
#endif
          }
#else
          if (f < wg_end) {
            uint32_t line = 0, col = 0;
            if (a.need_line) {  // uniform: some output is a field or 4:2:0
              line = __umulhi(f, a.magic_qpl);
              col = f - line * a.quads_per_line;
            }
#pragma unroll 1
#if PH_FM_BATCH
            for (uint32_t k = k0; k < k1; ++k) fused_out_store(outs[k], karg->plane[blockIdx.y][k], g, f, line, col);
#else
            for (uint32_t k = k0; k < k1; ++k) fused_out_store(outs[k], outs[k].plane, g, f, line, col);
#endif
          }
#endif
        }
      }
      k0 = k1;
    }
    __syncthreads();  // the next tile loads the reader's table
  }
#undef PH_FM_LUT_LOAD
