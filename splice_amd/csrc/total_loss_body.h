// The body of total_loss_kernel and total_loss_nn_kernel (step_engine.hip), included into both: the template flags MONITOR, TRACE, LRP, IMG,
// LYR, KG and NN, the kernels' parameters, and (NN) w_nn / nn_values are in scope at the point of inclusion.  One text, so that the
// instances without NN keep the code they had when the text stood in total_loss_kernel itself.
    static_assert(MONITOR || !LRP, "the lr rule rides on the stop rule");
    __shared__ float raw[8];
    float* l = lbase + (size_t)blockIdx.x * lstride;
    const int k = 1 + (threadIdx.x >> 6), lane = threadIdx.x & 63;   // wave k-1 owns term k (5 waves; 7 with IMG)
    const int n_slots = k == L_GLOBAL_SSIM ? n_a : k == L_GLOBAL_ID ? n_b : k == L_GLOBAL_CLS ? n_c : (IMG && k == L_GLOBAL_TV) ? n_a : (IMG && k == L_GLOBAL_PIX) ? n_b : n_e;
    const float* lp0 = lbase + (size_t)blockIdx.x * n_slots * lstride;   // the pair's first slot of this term
    float tot = 0.f;
    for (int slot = 0; slot < n_slots; ++slot) {
        const float* part = lp0 + (size_t)slot * lstride + 8 + (size_t)k * lp;
        if (LYR && (k == L_GLOBAL_SSIM || k == L_ENTIRE_SSIM)) {   // (wave-uniform: every lane walks the same slots)
            const int tiles = k == L_GLOBAL_SSIM ? tiles_g : tiles_e;
            float v = 0.f;
            for (int i = 0; i < n_layers; ++i) v += ssim_layer_sum(part + (size_t)i * tiles, tiles);
            tot += v;
            continue;
        }
        float acc = 0.f;
        for (int i = lane; i < lp; i += 64) acc += part[i];
        tot += wave_sum(acc);
    }
    const float acc = tot;
    if (lane == 0) raw[k] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        if (wtab) {
            const float* w = wtab + (size_t)blockIdx.x * 5;
            w_cls = w[0];
            w_ssim = ssim_on ? w[1] : 0.f;
            w_id = ssim_on ? w[2] : 0.f;
            w_ecls = entire ? w[3] : 0.f;
            w_essim = entire ? w[4] : 0.f;
        }
        for (int t = 1; t <= 5; ++t) l[t] = raw[t];
        // (the sum of five products with its contraction spelled out -- one product, then four fused multiply-adds: what the compiler made
        // of `w_ssim * raw_1 + w_essim * raw_2 + ...` in every instance before the lr rule, and would not make of it in the LRP instances)
        l[L_TOTAL] = __builtin_fmaf(w_id, raw[L_GLOBAL_ID], __builtin_fmaf(w_cls, raw[L_GLOBAL_CLS], __builtin_fmaf(w_ecls, raw[L_ENTIRE_CLS],
                         __builtin_fmaf(w_ssim, raw[L_GLOBAL_SSIM], w_essim * raw[L_ENTIRE_SSIM]))));
        if (IMG) {
            l[L_GLOBAL_TV] = raw[L_GLOBAL_TV]; l[L_GLOBAL_PIX] = raw[L_GLOBAL_PIX];
            l[L_TOTAL] = __builtin_fmaf(w_pix, raw[L_GLOBAL_PIX], __builtin_fmaf(w_tv, raw[L_GLOBAL_TV], l[L_TOTAL]));
        }
        if (KG) l[L_TOTAL] = __builtin_fmaf(w_kg, kg_values[blockIdx.x], l[L_TOTAL]);
        if (NN) l[L_TOTAL] = __builtin_fmaf(w_nn, nn_values[blockIdx.x], l[L_TOTAL]);
        if (out8) {   // the caller's losses buffer, written here instead of by a copy behind the step
            float* o = out8 + (size_t)blockIdx.x * 8;
            o[0] = l[L_TOTAL];
            for (int t = 1; t <= 5; ++t) o[t] = raw[t];
            o[6] = IMG ? raw[L_GLOBAL_TV] : 0.f; o[7] = IMG ? raw[L_GLOBAL_PIX] : 0.f;
        }
        if (TRACE) {
            const int row = *dev_t - 1;
            if (row >= 0 && row < capacity && !(MONITOR && stop_frozen(stop + blockIdx.x, row))) {
                float* tr = trace + ((size_t)row * gridDim.x + blockIdx.x) * 8;
                tr[0] = l[L_TOTAL];
                for (int t = 1; t <= 5; ++t) tr[t] = raw[t];
            }
        }
        if (LRP)
            lr_plateau_step(stop + blockIdx.x, lr_state + blockIdx.x, lr_cuts + (size_t)blockIdx.x * SPLICE_STOP_HISTORY, l[L_TOTAL], ssim_on && !entire, rule,
                            lr_rule, *dev_t - 1, lr_in[(size_t)blockIdx.x * lr_in_stride], lr_eff + blockIdx.x, kb ? kb + blockIdx.x : nullptr,
                            means ? means + (size_t)blockIdx.x * SPLICE_STOP_HISTORY : nullptr);
        else if (MONITOR && ssim_on && !entire)
            plateau_update(stop + blockIdx.x, l[L_TOTAL], rule, *dev_t - 1, kb ? kb + blockIdx.x : nullptr,
                           means ? means + (size_t)blockIdx.x * SPLICE_STOP_HISTORY : nullptr);
    }
