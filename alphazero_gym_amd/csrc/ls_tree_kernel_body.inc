// ls_tree_kernel_body.inc -- the body of ls_tree_kernel and ls_tree_kernel_nets (lockstep.cuh).  P: the kernel argument (the network's
// tensors, the trees, the tables); PT: what the tree phases read -- the same block, or a copy with the workgroup's net's MCTS settings.
    constexpr bool CONT = EnvFamily<ENV>::CONT;
    extern __shared__ double s_dyn[];   // sqrt_tab [tab_n], pw_need [n_sims+2]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, sub = lane & 15;
    const int tl = wave * 4 + (lane >> 4);
    const int tg = g_base + blockIdx.x;
    const int tree = tg * TREES_PER_WG + tl;
    const bool live = tree < P.B;
    const unsigned gtree = (unsigned)(P.tree_base + tree);
    double* s_sqrt = s_dyn;
    int* s_pw = (int*)(s_dyn + P.tab_n);
    for (int i = tid; i < P.tab_n; i += 256) s_sqrt[i] = P.sqrt_tab[i];
    if (CONT) for (int i = tid; i < P.n_sims + 2; i += 256) s_pw[i] = PT.pw_need[i];
    __syncthreads();
    const size_t tb = (size_t)(live ? tree : 0) * P.R;
    Cold* cold = P.cold + tb;
    double* edge_W = P.edge_W + tb;
    float* action = P.action + tb;
    TreeStore<TS_GLOBAL> ts;
    ts.hot = P.hot + tb;
    ts.child = P.child + tb * P.Kp;
    ts.prior = P.prior + tb;
    float* obsT = L.obsT + (size_t)tg * 64;
    TreeState st;
    if (sim == -2) {
        tree_init_root<ENV, TS_GLOBAL>(PT, st, ts, cold, edge_W, action, tree, live, sub, tl, gtree, obsT);
    } else {
        const LsTree t = L.tree[live ? tree : 0];
#ifdef AZG_STAMPS
        unsigned long long st_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // diagnostic build: discarded here
#endif
        const LsLane ln = L.lane[(size_t)(live ? tree : 0) * 16 + sub];
        st.nrec = t.nrec; st.eps_draws = t.eps_draws; st.leaf = t.leaf; st.need_eval = live && t.need_eval; st.path_D = t.path_D;
        st.kbase = t.kbase; st.my_depth = ln.my_depth; st.pid = ln.pid; st.pr = ln.pr; st.pW = ln.pW; st.eps_c = ln.eps_c;
        if (live) tree_phase_a<ENV, TS_GLOBAL, GMM, NCH>(PT, st, ts, cold, edge_W, action, tb, sim, sub, tl, gtree,
                                                     L.parts + (size_t)tg * NCH * 64, P.bhead + ls_net_wofs<POP>(P, tg), s_sqrt STAMP_ARG, s_pw);
        st.need_eval = false;
        if (sim < PT.n_sims - 1) {   // (PT: the net's own budget; the tables above are laid out for P.n_sims, the engine's)
            __threadfence_block();
            if (live) tree_phase_b<ENV, TS_GLOBAL, GMM>(PT, st, ts, cold, edge_W, action, tb, sub, tl, gtree, s_sqrt, s_pw, obsT STAMP_ARG);
            else if (sub < 4) obsT[sub * 16 + tl] = 0.0f;
        } else if (live && sub == 0) {
            P.n_rec[tree] = st.nrec;
        }
    }
    if (live) {
        if (sub == 0) {
            LsTree t;
            t.nrec = st.nrec; t.eps_draws = st.eps_draws; t.leaf = st.leaf; t.need_eval = st.need_eval ? 1 : 0; t.path_D = st.path_D;
            t.kbase = st.kbase;
            L.tree[tree] = t;
        }
        LsLane ln;
        ln.my_depth = st.my_depth; ln.pid = st.pid; ln.pr = st.pr; ln.pW = st.pW; ln.eps_c = st.eps_c; ln.pad = 0.0f;
        L.lane[(size_t)tree * 16 + sub] = ln;
    }
