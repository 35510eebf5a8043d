// engine_weights.hip -- the C ABI's weight uploads: from the caller's torch-layout blob to the kernels' operand layouts, for one network
// or the nets of a population (azg_set_population).
#include "engine_host.h"
#include "mlp.cuh"

extern "C" {

static int pad64(int n) { return (n + 63) / 64 * 64; }
static inline int unit_of(int i) { int t = i >> 4, r = (i >> 2) & 3, g = i & 3; return 16 * t + 4 * g + r; }

// ---- weights: from the caller's torch-layout blob to the kernels' operand layouts.
// The re-layout is a pure gather (every element of the engine's weight buffer is one element of the blob or a padding zero), so
// it is described ONCE per network shape by an index map (WeightMap::src: 1 + blob index, 0 = zero) and then applied either on the
// host (azg_set_weights: blob in host memory, one H2D copy of the result) or by a gather kernel (azg_set_weights_device: blob in
// device memory, e.g. the parameters PyTorch just updated or an RCCL broadcast buffer -- no host round trip).  Same map, same
// numbers, whichever side applies it.
static bool same_desc(const azg_mlp_desc& a, const azg_mlp_desc& b) {
    if (a.in_dim != b.in_dim || a.n_hidden != b.n_hidden || a.n_dist != b.n_dist || a.layernorm != b.layernorm) return false;
    for (int l = 0; l < a.n_hidden; ++l) if (a.hidden[l] != b.hidden[l]) return false;
    return true;
}

// validation shared by both entry points; HP_out = common padded hidden width, ncomp_out = mixture components (0: none)
static int check_desc(azg_engine* e, const azg_mlp_desc* d, size_t n_floats, int* HP_out, int* ncomp_out) {
    if (d->struct_size != (int32_t)sizeof(azg_mlp_desc)) return fail(e, AZG_E_INVALID, "azg_mlp_desc size mismatch");
    if (d->n_hidden < 1 || d->n_hidden > AZG_MAX_HIDDEN_LAYERS) return fail(e, AZG_E_INVALID, "n_hidden out of range");
    if (d->activation < 0 || d->activation > AZG_ACT_HARDSWISH) return fail(e, AZG_E_INVALID, "unknown activation");
    if (d->in_dim != e->S_obs) return fail(e, AZG_E_INVALID, "in_dim does not match the env observation");
    int ncomp = 0;
    if (e->cfg.mode == AZG_MODE_CONTINUOUS) {
        ncomp = d->num_components >= 2 ? d->num_components : 0;
        if (ncomp > 5) return fail(e, AZG_E_UNSUPPORTED, "at most 5 mixture components");
        if (d->n_dist != (ncomp ? 3 * ncomp : 2)) return fail(e, AZG_E_INVALID, "n_dist does not match num_components");
    } else if (d->n_dist != e->nd) return fail(e, AZG_E_INVALID, "n_dist does not match the engine mode");
    if (1 + d->n_dist > 16) return fail(e, AZG_E_UNSUPPORTED, "at most 15 distribution outputs");
    size_t need = 0;
    int k = d->in_dim, hmax = 0;
    for (int l = 0; l < d->n_hidden; ++l) {
        if (d->hidden[l] < 1 || d->hidden[l] > 4096) return fail(e, AZG_E_INVALID, "hidden width out of range");
        need += (size_t)d->hidden[l] * k + d->hidden[l] + (d->layernorm ? 2 * (size_t)d->hidden[l] : 0);
        k = d->hidden[l];
        if (k > hmax) hmax = k;
    }
    need += (size_t)(1 + d->n_dist) * k + (1 + d->n_dist);
    if (need != n_floats) return fail(e, AZG_E_INVALID, "weight blob size mismatch");
    const int HP = pad64(hmax);
    if (HP != 64 && HP != 128 && HP != 256 && HP != 512 && HP != 1024)
        return fail(e, AZG_E_UNSUPPORTED, "hidden width (padded to a multiple of 64) must be one of 64,128,256,512,1024");
    *HP_out = HP;
    *ncomp_out = ncomp;
    return AZG_OK;
}

// the index map of a network shape: where every element of the engine's weight buffer comes from
static void build_weight_map(const azg_mlp_desc* d, int HP, WeightMap& m) {
    typedef unsigned idx_t;   // 1 + index into the blob; 0: padding
    const int NT = HP / 16, S4 = HP / 16;
    // the blob's tensors as zero-padded [HP][Kp] index matrices (blob order = state_dict order: per layer weight, bias
    // (, LayerNorm weight, bias), then value head, distribution head)
    std::vector<std::vector<idx_t>> Wd(d->n_hidden), bd(d->n_hidden), gd(d->n_hidden), ed(d->n_hidden);
    idx_t p = 1;
    const int kp0 = d->in_dim > 4 ? 8 : 4;   // the first layer's input slots: one MFMA k-step, or two (five to eight inputs)
    int kt = d->in_dim, kp = kp0;
    for (int l = 0; l < d->n_hidden; ++l) {
        const int h = d->hidden[l];
        Wd[l].assign((size_t)HP * kp, 0);
        bd[l].assign(HP, 0);
        for (int n = 0; n < h; ++n)
            for (int kk = 0; kk < kt; ++kk) Wd[l][(size_t)n * kp + kk] = p + (idx_t)((size_t)n * kt + kk);
        p += (idx_t)((size_t)h * kt);
        for (int n = 0; n < h; ++n) bd[l][n] = p + n;
        p += h;
        gd[l].assign(HP, 0);
        ed[l].assign(HP, 0);
        if (d->layernorm) {
            for (int n = 0; n < h; ++n) gd[l][n] = p + n;
            p += h;
            for (int n = 0; n < h; ++n) ed[l][n] = p + n;
            p += h;
        }
        kt = h; kp = HP;
    }
    std::vector<idx_t> Wh((size_t)16 * HP, 0), bh(16, 0);
    for (int kk = 0; kk < kt; ++kk) Wh[kk] = p + kk;
    p += kt;
    bh[0] = p++;
    for (int o = 0; o < d->n_dist; ++o)
        for (int kk = 0; kk < kt; ++kk) Wh[(size_t)(1 + o) * HP + kk] = p + (idx_t)((size_t)o * kt + kk);
    p += (idx_t)((size_t)d->n_dist * kt);
    for (int o = 0; o < d->n_dist; ++o) bh[1 + o] = p + o;
    // MFMA operand layouts (lane l: row/col = l & 15, k-slot g = l >> 4; D register r of tile t = unit 16t + 4g + r); every
    // tensor starts 256-byte aligned in ONE buffer (one H2D copy / one gather per weight sync)
    std::vector<idx_t>& st = m.src;
    st.clear();
    auto reserve = [&](size_t n) { size_t off = st.size(); st.resize(off + (n + 63) / 64 * 64, 0); return off; };
    m.oW0 = reserve((size_t)NT * 64); m.ob0 = reserve((size_t)NT * 64 * 4);
    m.oW0b = reserve((size_t)NT * 64);        // inputs 4..7 (zeros for networks of at most four inputs)
    for (int t = 0; t < NT; ++t)
        for (int l = 0; l < 64; ++l) {
            const int row = 16 * t + (l & 15), g = l >> 4;
            st[m.oW0 + (size_t)t * 64 + l] = Wd[0][(size_t)row * kp0 + g];
            st[m.oW0b + (size_t)t * 64 + l] = kp0 == 8 ? Wd[0][(size_t)row * kp0 + 4 + g] : 0;
            for (int r = 0; r < 4; ++r) st[m.ob0 + ((size_t)t * 64 + l) * 4 + r] = bd[0][16 * t + 4 * g + r];
        }
    m.oW0u = reserve((size_t)HP * 4); m.ob0u = reserve((size_t)HP);
    for (int u = 0; u < HP; ++u) {   // (the VALU form of the first layer, team kernel: networks of at most four inputs only)
        for (int kk = 0; kk < 4; ++kk) st[m.oW0u + (size_t)u * 4 + kk] = Wd[0][(size_t)u * kp0 + kk];
        st[m.ob0u + u] = bd[0][u];
    }
    for (int l = 0; l < MAX_STREAM_LAYERS; ++l) { m.oWl[l] = m.obl[l] = m.olg[l] = m.olb[l] = 0; }
    for (int l = 1; l < d->n_hidden; ++l) {
        const size_t oW = reserve((size_t)NT * S4 * 64 * 4), ob = reserve((size_t)NT * 64 * 4);
        m.oWl[l - 1] = oW; m.obl[l - 1] = ob;
        for (int t = 0; t < NT; ++t)
            for (int l64 = 0; l64 < 64; ++l64) {
                const int row = 16 * t + (l64 & 15), g = l64 >> 4;
                for (int s4 = 0; s4 < S4; ++s4)
                    for (int j = 0; j < 4; ++j) {
                        const int i = 4 * (4 * s4 + j) + g;   // canonical position consumed by k-slot g of step 4*s4+j
                        st[oW + (((size_t)t * S4 + s4) * 64 + l64) * 4 + j] = Wd[l][(size_t)row * HP + unit_of(i)];
                    }
                for (int r = 0; r < 4; ++r) st[ob + ((size_t)t * 64 + l64) * 4 + r] = bd[l][16 * t + 4 * g + r];
            }
    }
    m.oWh = reserve((size_t)S4 * 64 * 4); m.obh = reserve(16);
    for (int s4 = 0; s4 < S4; ++s4)
        for (int l64 = 0; l64 < 64; ++l64) {
            const int o = l64 & 15, g = l64 >> 4;
            for (int j = 0; j < 4; ++j) {
                const int i = 4 * (4 * s4 + j) + g;
                st[m.oWh + ((size_t)s4 * 64 + l64) * 4 + j] = Wh[(size_t)o * HP + unit_of(i)];
            }
        }
    for (int o = 0; o < 16; ++o) st[m.obh + o] = bh[o];
    if (d->layernorm)
        for (int l = 0; l < d->n_hidden; ++l) {
            m.olg[l] = reserve((size_t)NT * 64 * 4); m.olb[l] = reserve((size_t)NT * 64 * 4);
            for (int t = 0; t < NT; ++t)
                for (int l64 = 0; l64 < 64; ++l64)
                    for (int r = 0; r < 4; ++r) {
                        st[m.olg[l] + ((size_t)t * 64 + l64) * 4 + r] = gd[l][16 * t + 4 * (l64 >> 4) + r];
                        st[m.olb[l] + ((size_t)t * 64 + l64) * 4 + r] = ed[l][16 * t + 4 * (l64 >> 4) + r];
                    }
        }
    m.desc = *d;
    m.HP = HP;
    m.valid = true;
}

__global__ __launch_bounds__(256) void weight_gather_kernel(const unsigned* __restrict__ src, const float* __restrict__ blob,
                                                            float* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { const unsigned s = src[i]; out[i] = s ? blob[s - 1] : 0.0f; }
}

// The population form: blockIdx.y = net k (of the nets written by one call) gathers blob k (blob + k * blob_stride) through the same
// map into its block of the engine's weight buffer (out + k * n): every net of a population in one launch.
__global__ __launch_bounds__(256) void weight_gather_nets_kernel(const unsigned* __restrict__ src, const float* __restrict__ blob,
                                                                 size_t blob_stride, float* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t k = blockIdx.y;
    if (i < n) { const unsigned s = src[i]; out[k * n + i] = s ? blob[k * blob_stride + s - 1] : 0.0f; }
}

// KParams' weight pointers: net 0's tensors in the engine's weight buffer (the kernels add net_wstride per net)
static void bind_weights(azg_engine* e, const WeightMap& m, const azg_mlp_desc* d) {
    const float* wb = e->d_wblob;
    e->P.net_wstride = e->n_nets > 1 ? m.src.size() : 0;
    e->P.W0u = (const f32x4*)(wb + m.oW0u);
    e->P.b0u = (const f32x4*)(wb + m.ob0u);
    e->P.W0 = wb + m.oW0;
    e->P.W0b = wb + m.oW0b;
    e->P.in8 = d->in_dim > 4 ? 1 : 0;
    e->P.b0 = (const f32x4*)(wb + m.ob0);
    for (int l = 0; l < MAX_STREAM_LAYERS; ++l) {
        const bool on = l + 1 < d->n_hidden;
        e->P.Wl[l] = on ? (const f32x4*)(wb + m.oWl[l]) : nullptr;
        e->P.bl[l] = on ? (const f32x4*)(wb + m.obl[l]) : nullptr;
    }
    e->P.Whead = (const f32x4*)(wb + m.oWh);
    e->P.bhead = wb + m.obh;
    e->P.layernorm = d->layernorm ? 1 : 0;
    for (int l = 0; l < MAX_STREAM_LAYERS; ++l) {
        e->P.Htrue[l] = l < d->n_hidden ? d->hidden[l] : 0;
        e->P.lng[l] = (d->layernorm && l < d->n_hidden) ? (const f32x4*)(wb + m.olg[l]) : nullptr;
        e->P.lnb[l] = (d->layernorm && l < d->n_hidden) ? (const f32x4*)(wb + m.olb[l]) : nullptr;
    }
}

// Continuous mode: the per-node mixture cache and the root-distribution staging buffer are sized by the head: rebuilt only when it
// changes (the last search's cached distributions go with them)
static int resize_head_buffers(azg_engine* e, const azg_mlp_desc* d, int ncomp) {
    if (e->cfg.mode != AZG_MODE_CONTINUOUS || (d->n_dist == e->dist_nd && ncomp == e->dist_ncomp)) return AZG_OK;
    e->dist_mem.clear();
    e->dist_nd = -1; e->searched = 0;
    float* g = nullptr;
    if (ncomp) { if (dalloc(e, e->dist_mem, &g, (size_t)e->cfg.n_trees * e->R * 3 * GMM_MAXC)) return AZG_E_DEVICE; }
    float* rd = nullptr;
    if (dalloc(e, e->dist_mem, &rd, (size_t)e->cfg.n_trees * d->n_dist)) return AZG_E_DEVICE;
    e->P.gmm = g; e->P.ncomp = ncomp; e->d_rootdist = rd; e->P.res_root_dist = rd; e->nd = d->n_dist; e->P.nd = d->n_dist;
    e->dist_nd = d->n_dist; e->dist_ncomp = ncomp;
    return AZG_OK;
}

// hidden->hidden layers that stay in the register file for the whole search (0: streamed)
static int resident_layers(const azg_engine* e, const azg_mlp_desc* d, int HP) {
    const int nhh = d->n_hidden - 1;
    const int regs = nhh * (HP * HP / 256);   // VGPRs per lane: each of the 4 waves holds a quarter of every layer
    // LayerNorm and the rare activations live in the weight-streaming kernels only (keeps the register-resident kernels lean)
    if (d->layernorm || (d->activation != AZG_ACT_RELU && d->activation != AZG_ACT_ELU) || e->opt.force_stream_weights) return 0;
    return (nhh >= 1 && nhh <= 2 && regs <= 288) ? nhh : 0;   // (three and more hidden->hidden layers: streamed, any depth)
}

// Common body of azg_set_weights / _device and the population uploads: `blob` is a host pointer (on_device false) or a device pointer
// whose contents are complete (its producer's stream synchronised or otherwise ordered before this call).
// `net`: which net of a population (azg_set_population) the weights are for; 0 for an engine of one net.  `n_write` nets net ..
// net + n_write - 1 are written from consecutive blobs of n_floats each (more than one: device blobs only, one gather launch).
static int set_weights_impl(azg_engine* e, const azg_mlp_desc* d, const float* blob, size_t n_floats, bool on_device, int net = 0,
                            int n_write = 1) {
    if (!e || !d || !blob) return AZG_E_INVALID;
    if (n_write != 1 && !on_device) return AZG_E_INVALID;
    int HP = 0, ncomp = 0;
    { int rc = check_desc(e, d, n_floats, &HP, &ncomp); if (rc) return rc; }
    const int NN = e->n_nets;
    bool others = false;   // a net of the population that keeps its weights already has some: they fix the descriptor
    for (int k = 0; k < NN; ++k) others = others || ((k < net || k >= net + n_write) && e->net_have[k]);
    if (NN > 1) {
        // decided by the descriptor alone, AZG_FORCE_PERSISTENT or not; the other wide shapes (LayerNorm, one hidden layer, more than
        // four inputs) run on the one-launch search kernel, any number of trees per net
        const int T = e->cfg.n_trees / NN;
        if (azg_lockstep_shaped(HP, d->n_hidden, d->layernorm != 0, d->in_dim) && T % 32 != 0)
            return fail(e, AZG_E_UNSUPPORTED, "populations of team / per-layer networks (padded width >= 512) need a multiple of 32 trees per net (got " +
                                              std::to_string(T) + "): a 32-tree team serves one net");
        if (others && !(e->wmap.valid && e->wmap.HP == HP && same_desc(e->wmap.desc, *d) && d->activation == e->wmap.desc.activation &&
                        d->num_components == e->wmap.desc.num_components && d->log_std_min == e->wmap.desc.log_std_min &&
                        d->log_std_max == e->wmap.desc.log_std_max))
            return fail(e, AZG_E_INVALID, "populations: every net must have the same network descriptor (azg_mlp_desc)");
    }
    ON_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    { int trc = settle_team(e); if (trc) return trc; }   // an abandoned team search is redone with the weights it was started with
    // nothing below may leave a half-updated weight set usable: the flag goes up again only on success
    e->mlp_ready = 0;
    e->results_valid = 0;
    e->redo_ok = 0;
    WeightMap& m = e->wmap;
    // the two weight sets (azgym_target.h) share the descriptor: one that differs in anything empties the set that is not in use
    if (!m.valid || m.HP != HP || !same_desc(m.desc, *d) || d->activation != m.desc.activation || d->num_components != m.desc.num_components ||
        d->log_std_min != m.desc.log_std_min || d->log_std_max != m.desc.log_std_max)
        e->w_idle.drop();
    if (!m.valid || m.HP != HP || !same_desc(m.desc, *d)) {
        m.valid = false;
        build_weight_map(d, HP, m);
        e->wmap_mem.clear(); e->d_wmap = nullptr;   // (uploaded when the device path first needs it)
    }
    m.desc = *d;
    // one block of n_out_f floats (a multiple of 64: every tensor starts 256-byte aligned) per net
    const size_t n_out_f = m.src.size();
    if (n_out_f != e->w_floats || !e->d_wblob) {
        e->wblob_mem.clear();
        e->d_wblob = nullptr; e->w_floats = 0;
        for (int k = 0; k < NN; ++k) e->net_have[k] = 0;   // (a new shape: the other nets' blocks no longer exist; NN > 1 cannot get here with any)
        if (dalloc(e, e->wblob_mem, &e->d_wblob, n_out_f * NN)) return AZG_E_DEVICE;
        e->w_floats = n_out_f;
    }
    float* const wnet = e->d_wblob + (size_t)net * n_out_f;
    for (int k = net; k < net + n_write; ++k) e->net_have[k] = 0;
    if (on_device) {
        if (!e->d_wmap) {
            if (dalloc(e, e->wmap_mem, &e->d_wmap, n_out_f)) return AZG_E_DEVICE;
            HIPCHK(e, hipMemcpy(e->d_wmap, m.src.data(), n_out_f * sizeof(unsigned), hipMemcpyHostToDevice));
        }
        if (n_write == 1)
            hipLaunchKernelGGL(weight_gather_kernel, dim3((unsigned)((n_out_f + 255) / 256)), dim3(256), 0, e->stream, e->d_wmap, blob, wnet, n_out_f);
        else
            for (int k0 = 0; k0 < n_write; k0 += 65535) {   // (grid.y is at most 65535)
                const int nk = n_write - k0 < 65535 ? n_write - k0 : 65535;
                hipLaunchKernelGGL(weight_gather_nets_kernel, dim3((unsigned)((n_out_f + 255) / 256), (unsigned)nk), dim3(256), 0, e->stream,
                                   e->d_wmap, blob + (size_t)k0 * n_floats, n_floats, wnet + (size_t)k0 * n_out_f, n_out_f);
            }
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipStreamSynchronize(e->stream));   // the caller may overwrite its blob as soon as this returns
    } else {
        std::vector<float>& st = e->w_stage;
        st.resize(n_out_f);
        const unsigned* src = m.src.data();
        for (size_t i = 0; i < n_out_f; ++i) st[i] = src[i] ? blob[src[i] - 1] : 0.0f;
        HIPCHK(e, hipMemcpy(wnet, st.data(), n_out_f * sizeof(float), hipMemcpyHostToDevice));
    }
    for (int k = net; k < net + n_write; ++k) e->net_have[k] = 1;
    bind_weights(e, m, d);
    { int rc = resize_head_buffers(e, d, ncomp); if (rc) return rc; }
    e->HP = HP; e->n_hidden = d->n_hidden;
    e->P.n_hidden = d->n_hidden; e->P.n_out = 1 + d->n_dist; e->P.act = d->activation; e->P.ls_min = d->log_std_min; e->P.ls_max = d->log_std_max;
    e->nreg = resident_layers(e, d, HP);
    bool all = true;
    for (int k = 0; k < NN; ++k) all = all && e->net_have[k];
    e->mlp_ready = all ? 1 : 0;   // (a population searches once every net has its weights)
    return AZG_OK;
}

static const char* kPopWeights = "this engine holds a population (azg_set_population > 1): upload each net's weights with azg_set_net_weights";

int azg_set_weights(azg_engine* e, const azg_mlp_desc* d, const float* blob, size_t n_floats) {
    if (e && e->n_nets > 1) return fail(e, AZG_E_STATE, kPopWeights);
    return set_weights_impl(e, d, blob, n_floats, false);
}

int azg_set_weights_device(azg_engine* e, const azg_mlp_desc* d, const float* device_blob, size_t n_floats) {
    if (e && e->n_nets > 1) return fail(e, AZG_E_STATE, kPopWeights);
    return set_weights_impl(e, d, device_blob, n_floats, true);
}

int azg_set_population(azg_engine* e, int32_t n_nets) {
    if (!e) return AZG_E_INVALID;
    if (n_nets < 1 || n_nets > e->cfg.n_trees || e->cfg.n_trees % n_nets != 0)
        return fail(e, AZG_E_INVALID, "azg_set_population: n_nets must divide n_trees (trees k*T .. k*T+T-1 belong to net k, T = n_trees / n_nets)");
    if (e->ring.on) return fail(e, AZG_E_UNSUPPORTED, "azg_set_population: device self-play is running on this engine (one network per engine)");
    if (n_nets == e->n_nets) return AZG_OK;
    ON_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    { int trc = settle_team(e); if (trc) return trc; }
    // the diagnostic stamp buffer has a row per wave of the grid, which padding every net's segment to whole workgroups enlarges
    // (stamp_rows of the 16-tree padded count covers the 8-, 16- and 32-tree shapes)
    const size_t rows = stamp_rows((size_t)n_nets * (((size_t)e->cfg.n_trees / n_nets + 15) / 16 * 16));
    if (rows > e->stamp_n) {
        DeviceAllocs bigger;
        unsigned long long* st = nullptr;
        if (dalloc(e, bigger, &st, rows * 16)) return AZG_E_DEVICE;
        e->stamp_mem.ptrs.swap(bigger.ptrs);   // (the old buffer goes with `bigger`)
        e->P.stamps = st; e->stamp_n = rows;
    }
    // every weight goes: the next search needs the weights of every net again
    e->wblob_mem.clear();
    e->d_wblob = nullptr; e->w_floats = 0;
    e->w_idle.drop();   // (the set that is not in use, azgym_target.h, was laid out for the old split too)
    // ... and so do per-net search settings: their table has one entry per net of the old split
    e->net_search = NetSearchTable{};
    e->net_search_mem.clear();
    e->net_search_wide = 0;
    e->net_sims_max = 0;
    e->net_search_gamma.clear();
    e->n_nets = n_nets;
    e->net_have.assign(n_nets, 0);
    e->mlp_ready = 0; e->results_valid = 0; e->redo_ok = 0; e->searched = 0;
    e->P.net_T = e->cfg.n_trees / n_nets; e->P.net_wstride = 0;
    return AZG_OK;
}

// Per-net MCTS settings: validated on the host, then one record and one widening table per net on the device (records.h:
// NetSearchTable).  The buffers are allocated when the table appears and reused while it stays; the copies go on the engine's stream,
// behind whatever search is running there.  wide: the table may be searched at padded widths >= 512 (AZG_NET_SEARCH_WIDE); a call that
// fails leaves the table and its permission as they were.
// Budgets: azg_net_search::n_sims (0: the engine's) is the net's own number of simulations, at most azg_config's, which stays the
// capacity everything was sized for at creation.  The net's widening table is built with its own budget -- the entries a one-net engine
// created with that budget builds, the rest of its capacity-sized row zero and never read (tree.cuh: pw_at clamps at the budget + 1) --
// and its Kmax check counts the children its own budget reaches.
static int set_net_search(azg_engine* e, const azg_net_search* nets, int32_t n_nets, bool wide) {
    const bool clear = !nets || n_nets == 0;
    const bool cont = e->cfg.mode == AZG_MODE_CONTINUOUS;
    const int ns = e->cfg.n_sims;
    std::vector<NetSearchRec> rec;
    std::vector<int> pw_all, pw;
    int sims_max = 0;
    if (!clear) {
        if (n_nets != e->n_nets)
            return fail(e, AZG_E_INVALID, "azg_set_net_search: n_nets must equal the engine's number of nets (azg_set_population): got " +
                                          std::to_string(n_nets) + ", the engine has " + std::to_string(e->n_nets));
        rec.resize(n_nets);
        pw_all.assign((size_t)n_nets * (ns + 2), 0);
        for (int k = 0; k < n_nets; ++k) {
            const azg_net_search& s = nets[k];
            const std::string who = "azg_set_net_search: net " + std::to_string(k) + ": ";
            if (s.struct_size != (int32_t)sizeof(azg_net_search)) return fail(e, AZG_E_INVALID, who + "azg_net_search size mismatch");
            if (!std::isfinite(s.c_uct) || !std::isfinite(s.gamma) || !std::isfinite(s.epsilon))
                return fail(e, AZG_E_INVALID, who + "c_uct, gamma and epsilon must be finite");
            if (s.n_sims < 0 || s.n_sims > ns)
                return fail(e, AZG_E_INVALID, who + "n_sims must be 0 (the engine's) or 1 .. " + std::to_string(ns) + ", the n_sims the engine was created "
                                              "with (its capacity): got " + std::to_string(s.n_sims));
            const int ns_k = s.n_sims ? s.n_sims : ns;
            if (ns_k > sims_max) sims_max = ns_k;
            NetSearchRec& r = rec[k];
            r.c_uct = s.c_uct; r.gamma = s.gamma; r.epsilon = s.epsilon;
            r.c_uct_f = (float)s.c_uct; r.gamma_f = (float)s.gamma;
            r.c_pw = 0.0; r.kappa = 0.0; r.pw0 = 0; r.n_sims = ns_k;
            if (!cont) continue;   // (discrete mode: no widening)
            if (!azg_pw_params_ok(s.c_pw, s.kappa))
                return fail(e, AZG_E_INVALID, who + "c_pw must be > 0 and kappa >= 0 (progressive widening: ceil(c_pw (n + 1)^kappa) children)");
            // the trees, the child lists and the results were sized at creation for azg_config's widening: every net must stay inside
            const int kmax = azg_pw_table(s.c_pw, s.kappa, ns_k, pw);   // (ns_k + 2 entries)
            if (kmax > e->Kmax)
                return fail(e, AZG_E_INVALID, who + "its widening (c_pw, kappa) entitles a node to " + std::to_string(kmax) + " children, the engine was "
                                              "created for at most " + std::to_string(e->Kmax) + " (azg_max_children): create it with the widest net's c_pw / kappa");
            r.c_pw = s.c_pw; r.kappa = s.kappa; r.pw0 = pw[0];
            std::copy(pw.begin(), pw.end(), pw_all.begin() + (size_t)k * (ns + 2));
        }
    }
    ON_DEVICE(e);
    { int trc = settle_team(e); if (trc) return trc; }   // an abandoned team search is redone with the settings it was started with
    e->redo_ok = 0;   // (azg_dump_tree re-runs a search only while its inputs stand: the table is one of them)
    if (clear) {
        if (!e->net_search.rec) return AZG_OK;
        HIPCHK(e, hipStreamSynchronize(e->stream));   // a running search still reads the table
        e->net_search = NetSearchTable{};
        e->net_search_mem.clear();
        e->net_search_wide = 0;
        e->net_sims_max = 0;
        e->net_search_gamma.clear();
        return AZG_OK;
    }
    if (!e->net_search.rec) {
        NetSearchRec* d_rec = nullptr; int* d_pw = nullptr;
        if (dalloc(e, e->net_search_mem, &d_rec, (size_t)n_nets) || dalloc(e, e->net_search_mem, &d_pw, pw_all.size())) {
            e->net_search_mem.clear();
            return AZG_E_DEVICE;
        }
        e->net_search.rec = d_rec; e->net_search.pw_need = d_pw;
    }
    HIPCHK(e, hipMemcpyAsync((void*)e->net_search.rec, rec.data(), rec.size() * sizeof(NetSearchRec), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync((void*)e->net_search.pw_need, pw_all.data(), pw_all.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));   // (the staging vectors go when this returns)
    e->net_search_wide = wide ? 1 : 0;
    e->net_sims_max = sims_max;
    e->net_search_gamma.resize(n_nets);
    for (int k = 0; k < n_nets; ++k) e->net_search_gamma[k] = rec[k].gamma;
    return AZG_OK;
}

int azg_set_net_search(azg_engine* e, const azg_net_search* nets, int32_t n_nets) {
    if (!e) return AZG_E_INVALID;
    return set_net_search(e, nets, n_nets, false);
}

int azg_set_net_search_ex(azg_engine* e, const azg_net_search* nets, int32_t n_nets, uint32_t flags) {
    if (!e) return AZG_E_INVALID;
    if (flags & ~(uint32_t)AZG_NET_SEARCH_WIDE) return fail(e, AZG_E_INVALID, "azg_set_net_search_ex: unknown flag bits (AZG_NET_SEARCH_WIDE is the only flag)");
    return set_net_search(e, nets, n_nets, (flags & AZG_NET_SEARCH_WIDE) != 0);
}

// ---- the second weight set (include/azgym_target.h).  The set in use is what d_wblob / w_floats / net_have / mlp_ready describe, so
// every upload above writes it and bind_weights points the kernels at it; selecting the other set swaps those with the parked ones.
int azg_use_weights(azg_engine* e, int32_t which) {
    if (!e) return AZG_E_INVALID;
    if (which != AZG_WEIGHTS_LIVE && which != AZG_WEIGHTS_TARGET)
        return fail(e, AZG_E_INVALID, "azg_use_weights: which must be AZG_WEIGHTS_LIVE or AZG_WEIGHTS_TARGET");
    if (which == e->w_in_use) return AZG_OK;
    ON_DEVICE(e);
    { int trc = settle_team(e); if (trc) return trc; }   // an abandoned team search is redone with the weights it was started with
    IdleWeights& o = e->w_idle;
    if (o.have.size() != (size_t)e->n_nets) o.have.assign(e->n_nets, 0);   // (a set nothing was uploaded to since it was emptied)
    e->wblob_mem.ptrs.swap(o.mem.ptrs);
    std::swap(e->d_wblob, o.blob);
    std::swap(e->w_floats, o.floats);
    e->net_have.swap(o.have);
    std::swap(e->mlp_ready, o.ready);
    e->w_in_use = which;
    // launches already made hold their weight pointers by value: no synchronisation.  What is cached about the last search goes, as
    // after an upload
    e->results_valid = 0;
    e->redo_ok = 0;
    if (e->d_wblob) bind_weights(e, e->wmap, &e->wmap.desc);
    return AZG_OK;
}

int azg_weights_info(const azg_engine* e, int32_t* in_use, int32_t* target_ready) {
    if (!e) return AZG_E_INVALID;
    if (in_use) *in_use = e->w_in_use;
    if (target_ready) *target_ready = e->w_in_use == AZG_WEIGHTS_TARGET ? e->mlp_ready : e->w_idle.ready;
    return AZG_OK;
}

int azg_set_net_weights(azg_engine* e, int32_t net, const azg_mlp_desc* d, const float* blob, size_t n_floats) {
    if (!e) return AZG_E_INVALID;
    if (net < 0 || net >= e->n_nets) return fail(e, AZG_E_INVALID, "azg_set_net_weights: net index out of range");
    return set_weights_impl(e, d, blob, n_floats, false, net);
}

int azg_set_net_weights_device(azg_engine* e, int32_t net, const azg_mlp_desc* d, const float* device_blob, size_t n_floats) {
    if (!e) return AZG_E_INVALID;
    if (net < 0 || net >= e->n_nets) return fail(e, AZG_E_INVALID, "azg_set_net_weights_device: net index out of range");
    return set_weights_impl(e, d, device_blob, n_floats, true, net);
}

int azg_set_population_weights_device(azg_engine* e, const azg_mlp_desc* d, const float* device_blobs, size_t n_floats_per_net, int32_t n_nets) {
    if (!e) return AZG_E_INVALID;
    if (n_nets != e->n_nets)
        return fail(e, AZG_E_INVALID, "azg_set_population_weights_device: n_nets must equal the engine's number of nets (azg_set_population)");
    return set_weights_impl(e, d, device_blobs, n_floats_per_net, true, 0, n_nets);
}

}  // extern "C"
