// env_step_body.inc -- the env kernel's body: one launch's work of a workgroup on its kArenas arenas.  Included as
// text where `g` (StepArgs) and `lds` (__shared__ ArenaLDS [kArenas]) are in scope: by the per-step kernel as its
// whole body, and by the collection loop kernel once per step (env_step.hpp).  Text, not a device function: the
// per-step kernel then compiles to exactly the code it had when the body stood in it.
    const int team = threadIdx.x >> 4, l = threadIdx.x & 15;
    const int arena = blockIdx.x * kArenas + team;
    const bool valid = arena < g.n;
    ArenaLDS* A = &lds[team];
    Prof P{g.prof, g.prof ? (long long)clock64() : 0};
    // ---- stage the 4 arena records into LDS (contiguous 16-byte loads)
    {
        int first = blockIdx.x * kArenas;
        int cnt = g.n - first < kArenas ? g.n - first : kArenas;
        const int chunks = kRec / 16;
        for (int k = threadIdx.x; k < cnt * chunks; k += kWG) {
            int a = k / chunks, c = k % chunks;
            const uint4* src = (const uint4*)(g.arenas + (size_t)(first + a) * kRec) + c;
            uint4* dst = (uint4*)&lds[a] + c;
            *dst = *src;
        }
    }
    sync(); P.mark(11);
    RLGPU_BODY_STAMP(kSplitLoad)  // empty but in the collection loop's profiled instantiation (env_step.hpp)
    if (valid && l < 5) {
        A->a.force[l] = zero3();
        A->a.torque[l] = zero3();
        update_inertia(A, l);
    }
    if (l == 0) {
        A->a.epa_lock = A->a.npen = 0;
        A->a.arith = g.arith;
    }
    if (threadIdx.x == 0) g_pen_save.cap = g.pen_slots;
    sync(); P.mark(11);
    // ---- StepFirstHalf (EnvSet.cpp:113-130) prelude
    if (g.ticks_first > 0) {
        if (valid && l == 0) {
            rlgpu_env_extra& e = A->s.env;
            for (int i = 0; i < 3; i++) e.prev_ball_vel[i] = A->s.ball.vel[i] * kBT2UU;
            for (int i = 0; i < 4; i++) {
                e.prev_boost[i] = A->s.cars[i].boost;
                e.prev_is_flipping[i] = A->s.cars[i].is_flipping;
                e.prev_on_ground[i] = A->s.cars[i].is_on_ground;
                e.ev_bump[i] = e.ev_bumped[i] = e.ev_demo[i] = e.ev_demoed[i] = 0;
            }
            e.has_prev = 1;
        }
        sync(); P.mark(11);
    }
    // ---- the ticks of both halves in ONE loop (a single inlined copy of the tick body keeps the
    // kernel's hot code small enough for the instruction cache); StepSecondHalf's action parse
    // (EnvSet.cpp:132-156) runs when the first half's actionDelay ticks are done
    {
        PadRegs pregs;
        load_pad_regs(pregs, l);
        const int t1 = g.ticks_first, t2 = g.actions ? g.ticks_second : 0;
        for (int t = 0;; t++) {
            if (g.actions && t == t1) {
                if (valid && l < 4) {
                    int a = g.actions[arena * 4 + l];
                    a = a < 0 ? 0 : (a > RLGPU_ACTIONS - 1 ? RLGPU_ACTIONS - 1 : a);
                    const float* x = C.action[a];
                    float* c = A->s.cars[l].controls;
                    for (int k = 0; k < 5; k++) c[k] = x[k];
                    c[5] = x[5] == 1 ? 1.f : 0.f;
                    c[6] = x[6] == 1 ? 1.f : 0.f;
                    c[7] = x[7] == 1 ? 1.f : 0.f;
                    for (int k = 0; k < 8; k++) A->s.env.prev_action[l][k] = x[k];
                }
                sync(); P.mark(11);
            }
            if (t >= t1 + t2) break;
            tick(A, g.mesh, l, valid, g.seed, arena + g.arena_offset, P, pregs, stdmin(kArenas, g.n - (int)blockIdx.x * kArenas));
        }
    }
    // ---- builders: GameState::UpdateFromArena, terminals, rewards, obs, masks
    uint8_t term = 0;
    if (g.build) {
        if (valid && l == 0) {
            rlgpu_env_extra& e = A->s.env;
            int64_t cur = e.tick_count;
            int64_t tick_skip = cur - e.last_tick_count > 0 ? cur - e.last_tick_count : 0;
            float delta_time = (int)tick_skip * (1.0f / 120.0f);
            bool any = false;
            for (int i = 0; i < 4; i++) {
                const rlgpu_car& c = A->s.cars[i];
                bool t = c.ball_hit_valid && (uint64_t)c.ball_hit_tick >= (uint64_t)(cur - tick_skip);
                A->a.touched[i] = t;
                any |= t;
            }
            float by = A->s.ball.pos[1] * kBT2UU;
            bool goal = fabsf(by) > (5124.25f + 91.25f);
            A->a.goal = goal;
            // the conditions' state: NoTouchCondition::timeSinceTouch and ScoreLimitCondition's goal
            // counts evolve identically in every instance (each IsTerminal is called every step), so one
            // copy serves any number of instances with different limits
            if (any) e.no_touch_time = 0;
            else e.no_touch_time += delta_time;
            if (goal) {
                if (by > 0) e.score_blue++;
                else e.score_orange++;
            }
            // terminal merge over the registry's list (EnvSet.cpp:167-180): NORMAL dominates
            uint8_t tt = 0;
            for (int k = 0; k < g.plug->nt; k++) {
                const rlgpu_terminal_spec& tc = g.plug->tc[k];
                bool hit = false, trunc = false;
                if (tc.type == RLGPU_TC_NO_TOUCH) {
                    hit = !any && e.no_touch_time >= tc.param;
                    trunc = true;
                } else if (tc.type == RLGPU_TC_SCORE_LIMIT) {
                    const int lim = (int)tc.param;
                    hit = (e.score_blue >= lim) || (e.score_orange >= lim);
                } else if (tc.type == RLGPU_TC_GOAL_SCORE) {
                    hit = goal;
                }
                if (hit) {
                    const uint8_t cur = trunc ? 2 : 1;
                    if (tt == 0 || cur == 1) tt = cur;
                }
            }
            e.terminal = tt;
            if (goal) {
                if (by > 0) e.penalty_blue++;
                else e.penalty_orange++;
            }
            // trajectory-level code (Learner.cpp:829-861): max episode length truncates the
            // trajectory without resetting the arena
            e.episode_steps++;
            uint8_t tj = tt;
            if (!tj && g.max_episode_steps > 0 && e.episode_steps >= g.max_episode_steps) tj = 2;
            if (tj) e.episode_steps = 0;
            A->a.traj_term = tj;
        }
        sync(); P.mark(12);
        if (valid) {
            // the arena's 16 lanes: lane l evaluates player l & 3's rewards r = l >> 2, + 4, + 8, ... (each reward is a
            // pure function of the snapshot); then the player's lane sums them in list order, allRewards[i] +=
            // out[i] * weight (EnvSet.cpp:199-222), fetching each value from the lane that computed it
            const int pi = l & 3, q = l >> 2;
            const PView me = view_player(A, pi);  // the other players' views are read where used
            v3 bp = ld3(A->s.ball.pos) * kBT2UU, bv = ld3(A->s.ball.vel) * kBT2UU, pbv = ld3(A->s.env.prev_ball_vel);
            const int nr = g.plug->nr;
            constexpr int kPer = (RLGPU_MAX_REWARDS + 3) / 4;
            float ov[kPer];
#pragma unroll
            for (int k = 0; k < kPer; k++) ov[k] = 0.f;
#pragma unroll 1
            for (int k = 0; q + 4 * k < nr; k++) {
                const int r = q + 4 * k;
                const float o = reward_value(A, g.plug->rw[r], pi, me, bp, bv, pbv, A->a.goal != 0);
#pragma unroll
                for (int j = 0; j < kPer; j++) ov[j] = j == k ? o : ov[j];  // no run-time register index
                if (pi == 0 && g.last_rewards) g.last_rewards[(size_t)arena * nr + r] = o;
                if (g.reward_values) g.reward_values[((size_t)arena * 4 + pi) * nr + r] = o;
            }
            float all = 0.f;
            const int base = (int)(threadIdx.x & ~15u) + pi;
#pragma unroll
            for (int r = 0; r < RLGPU_MAX_REWARDS; r++) {
                if (r >= nr) break;
                const float o = __shfl(ov[r >> 2], base + 4 * (r & 3));
                all += o * g.plug->rw[r].weight;
            }
            if (l < 4) A->a.all_rewards[l] = all;
        }
        sync(); P.mark(12);
        if (valid && l < 4) {
            float r = A->a.all_rewards[l];
            g.rewards[arena * 4 + l] = r;
            if (g.out_rew) g.out_rew[arena * 4 + l] = r;
            if (g.out_term) g.out_term[arena * 4 + l] = (int8_t)A->a.traj_term;
        }
        if (g.metrics && valid && l < 4) step_metrics(A, l, g.metrics + (size_t)arena * RLGPU_STEP_METRIC_SLOTS,
                                                      g.metrics_players != 0);
        uint8_t tj = 0;
        if (valid) {
            term = A->s.env.terminal;
            tj = (uint8_t)A->a.traj_term;
        }
        sync(); P.mark(12);
        if (valid && l == 0) {
            g.terminals[arena] = term;
            A->s.env.last_tick_count = A->s.env.tick_count;
        }
        const bool fused_reset = g.reset_mode == kResetTerminated && valid && term != 0;
        if (valid) build_obs_rows(A, g.plug, l, arena + g.arena_offset);
        sync(); P.mark(13);
        if (valid) {
            copy_rows(A, g.plug, l, arena, g.obs, g.masks);
            if (!fused_reset) copy_rows(A, g.plug, l, arena, g.out_obs, g.out_masks);
            if (tj == 2) {
                copy_rows(A, g.plug, l, arena, g.trunc_obs, nullptr);
                copy_rows(A, g.plug, l, arena, g.out_trunc, nullptr);
            }
        }
        sync(); P.mark(13);
        if (g.reset_mode == kResetTerminated) {
            if (fused_reset && l == 0) state_reset(A, g.plug, g.seed, arena + g.arena_offset);
            sync(); P.mark(14);
            if (fused_reset) build_obs_rows(A, g.plug, l, arena + g.arena_offset);
            sync(); P.mark(14);
            if (fused_reset) {
                copy_rows(A, g.plug, l, arena, g.obs, g.masks);
                copy_rows(A, g.plug, l, arena, g.out_obs, g.out_masks);
            }
            sync(); P.mark(14);
        }
    }
    // ---- EnvSet::Reset / ResetArena / obs rebuild
    if (g.reset_mode >= kResetSet) {
        bool do_reset = false;
        if (valid) {
            if (g.reset_mode == kResetSet) do_reset = g.terminals[arena] != 0;
            else if (g.reset_mode == kResetMask) do_reset = g.reset_mask ? g.reset_mask[arena] != 0 : true;
            else if (g.reset_mode == kResetAll) do_reset = true;
        }
        sync(); P.mark(14);
        if (do_reset && l == 0) {
            state_reset(A, g.plug, g.seed, arena + g.arena_offset);
            if (g.reset_mode == kResetSet) g.terminals[arena] = 0;
        }
        sync(); P.mark(14);
        bool rebuild = do_reset || (valid && g.reset_mode == kRebuildObs);
        if (rebuild) build_obs_rows(A, g.plug, l, arena + g.arena_offset);
        sync(); P.mark(14);
        if (rebuild) copy_rows(A, g.plug, l, arena, g.obs, g.masks);
        sync(); P.mark(14);
    }
    // ---- write the records back
    RLGPU_BODY_STAMP(kSplitBody)
    {
        int first = blockIdx.x * kArenas;
        int cnt = g.n - first < kArenas ? g.n - first : kArenas;
        const int chunks = kRec / 16;
        for (int k = threadIdx.x; k < cnt * chunks; k += kWG) {
            int a = k / chunks, c = k % chunks;
            uint4* dst = (uint4*)(g.arenas + (size_t)(first + a) * kRec) + c;
            const uint4* src = (const uint4*)&lds[a] + c;
            *dst = *src;
        }
    }
    P.mark(15);
    if (g.prof && valid && l == 0 && A->a.npen) {  // penetration-solver calls: total and this workgroup's
        atomicAdd(&g.prof[28], (unsigned long long)A->a.npen);
        atomicAdd(&g.prof[kProfWG + (size_t)blockIdx.x * kProfPhases + 23], (unsigned long long)A->a.npen);
        atomicAdd(&g.prof[kProfWG + (size_t)gridDim.x * kProfPhases + arena], (unsigned long long)A->a.npen);
    }
