/*
 * oc_engine.h -- C-ABI of the MI355X batched Overcooked step engine (liboc_engine.so).
 *
 * The reference (deletfsi/gym-cooking) is pure Python and has no FFI; each entry point
 * below replaces one reference routine on the environment-step hot path and is what a
 * ctypes/cffi binding of that routine binds (INTEGRATION.md shows the binding):
 *
 *   oc_create / oc_destroy   <- OvercookedEnvironment.load_level + run_recipes
 *                               (gym_cooking/envs/overcooked_environment.py:130-198, :396-473)
 *   oc_reset                 <- OvercookedEnvironment.reset      (overcooked_environment.py:201-250)
 *   oc_step, oc_step_n       <- OvercookedEnvironment.step       (overcooked_environment.py:255-306)
 *                               = check_collisions (:724-762) + execute_navigation/interact
 *                               (:767-770, gym_cooking/utils/interact.py:4-89) + done/reward (:316-376)
 *   oc_observe, oc_cpu_observe <- a grid encoding of world.objects / sim_agents (utils/core.py:28-305) and
 *                               get_single_actions (gym_cooking/navigation_planner/utils.py:55-90) per agent
 *   oc_progress, oc_cpu_progress <- RealAgent.def_subtask_completion / is_subtask_complete
 *                               (gym_cooking/utils/agent.py:286-368) for every subtask of a recipe, per env
 *   oc_reset_random, oc_cpu_reset_random, oc_set_start_cells, oc_get_start_cells
 *                            <- load_level (:144-193) + reset (:201-250) of the level file with its item
 *                               letters and spawn lines moved, per env
 *   oc_nav_policy, oc_cpu_nav_policy <- a Boltzmann-rational agent following a subtask: the action model
 *                               BayesianDelegator.prob_nav_actions scores
 *                               (gym_cooking/delegation_planner/bayesian_delegator.py:461-689), sampled
 *   oc_gen_actions           <- synthetic action streams (the reference env has no RNG)
 *   oc_stats_*               <- the per-episode bookkeeping main.py keeps in its metrics Bag
 *                               (gym_cooking/misc/metrics/metrics_bag.py:40-72), reduced per GPU
 *
 * Conventions
 *  - All entry points return 0 on success and a negative OC_E* code on failure; the message
 *    of the last failure on the calling thread is available from oc_last_error(), and the
 *    last failure of a call on a given handle from oc_get_last_error(h, buf, size).
 *  - Every buffer is caller-owned device memory (e.g. torch ROCm tensors); the engine never
 *    allocates in oc_step / oc_reset / oc_gen_actions, so they are hipGraph-capturable.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls are
 *    stream-ordered and not synchronised; a handle is not thread-safe.
 *  - State is structure-of-arrays: `num_planes` byte planes of `pitch` bytes each (see
 *    oc_layout).  Env e of plane p lives at byte p*pitch + e (the t plane holds u16 at
 *    2*e and spans two planes).  pitch = B rounded up to OC_PITCH_ALIGN.
 *  - Columns [B, pitch) of an output plane belong to the engine: the step kernels move four
 *    envs per 32-bit word, so the columns of the batch's last word past B may be rewritten
 *    (the state planes with what the input held there or its step, exec_actions / coll_mask
 *    with no-op / 0).  Nothing at or past the next multiple of 4 above B is written, and no
 *    statistic counts a column past B.
 */
#ifndef OC_ENGINE_H_
#define OC_ENGINE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OC_ABI_VERSION 12

#define OC_MAX_AGENTS 4
#define OC_MAX_ITEMS 16  /* item slots: K = 4, 8 or 16 per level */
#define OC_MAX_CELLS 1024       /* grid cells (width and height <= 255 each) */
#define OC_MAX_NARROW_CELLS 255 /* levels of at most this many cells have byte cell ids (0xFF is
                                   OC_LOC_DEAD); larger ("wide") levels u16 ids (OC_LOC_DEAD16) */
#define OC_MAX_GOALS 4
#define OC_PITCH_ALIGN 4096

/* status codes */
#define OC_OK 0
#define OC_EINVAL (-1)   /* bad argument / unsupported shape */
#define OC_EHIP (-2)     /* HIP runtime error */
#define OC_ELEVEL (-3)   /* level outside the exact-semantics envelope */

/* tile classes (gym_cooking/utils/core.py:28-120; only Floor is non-collidable) */
#define OC_TILE_FLOOR 0
#define OC_TILE_COUNTER 1
#define OC_TILE_CUTBOARD 2
#define OC_TILE_DELIVERY 3

/* Item content masks, two encodings (oc_level_desc.encoding).
 * OC_ENC_PRESENCE: presence T,L,O,P + chopped T,L,O; exact for levels with at
 *   most one of each food type (every shipped level).
 * OC_ENC_COUNTS: the multiset of a core.Object's contents (equality is by full_name, a sorted
 *   multiset: gym_cooking/utils/core.py:143-171): a 2-bit count per food, a plate bit and a
 *   Fresh bit.  Exact for levels with up to 3 of each food type (load_level makes one Object
 *   per map character with no uniqueness check, overcooked_environment.py:158-165): an object
 *   of more than one content is a merge, and mergeable() (core.py:222-241) admits only foods
 *   in their last state and at most one plate, so a merged object is all-Chopped and the
 *   Fresh bit only ever marks a single fresh food.  Goal masks never carry it. */
#define OC_M_TOMATO 0x01u
#define OC_M_LETTUCE 0x02u
#define OC_M_ONION 0x04u
#define OC_M_PLATE 0x08u
#define OC_M_CHOPPED_SHIFT 4
#define OC_ENC_PRESENCE 0
#define OC_ENC_COUNTS 1
#define OC_MC_TOMATO 0x01u   /* count field bits 0-1 */
#define OC_MC_LETTUCE 0x04u  /* bits 2-3 */
#define OC_MC_ONION 0x10u    /* bits 4-5 */
#define OC_MC_PLATE 0x40u
#define OC_MC_FRESH 0x80u    /* a single food in its Fresh state */
#define OC_MC_MAX_PER_FOOD 3

/* action codes: World.NAV_ACTIONS order (gym_cooking/utils/world.py:16) + no-op.
 * Codes > 4 are treated as OC_ACT_NOOP. */
#define OC_ACT_DOWN 0   /* ( 0, 1) */
#define OC_ACT_UP 1     /* ( 0,-1) */
#define OC_ACT_LEFT 2   /* (-1, 0) */
#define OC_ACT_RIGHT 3  /* ( 1, 0) */
#define OC_ACT_NOOP 4   /* ( 0, 0) */

#define OC_HOLD_NONE 0xFFu
#define OC_LOC_DEAD 0xFFu
#define OC_LOC_DEAD16 0xFFFFu

/* flags plane bits */
#define OC_FLAG_DONE 0x01u    /* done() returned True (overcooked_environment.py:316-363) */
#define OC_FLAG_SUCCESS 0x02u /* reward() == 1 (overcooked_environment.py:365-376) */
#define OC_FLAG_ERR 0x04u     /* the reference's step raises: at new_obs = copy.copy(self)
                                 (overcooked_environment.py:289 -> world.py:417) when two
                                 co-located agents both hold, or, on a level with a Floor on its
                                 border and two or more agents, in check_collisions when an action
                                 points off the grid (is_collision :692-700 -> get_gridsquare_at
                                 asserts, world.py:429; the state is then unchanged but t, the
                                 executed actions no-ops).  ERR implies DONE. */

/* per-GPU episode statistics (oc_stats_reduce output, uint64 each) */
#define OC_STAT_EPISODES 0   /* envs whose episode ended this window (DONE newly set) */
#define OC_STAT_SUCCESSES 1  /* of those, reward 1 */
#define OC_STAT_STEPS 2      /* sum of t over ended episodes (episode lengths) */
#define OC_STAT_COLLISIONS 3 /* sum over steps of colliding agent pairs (CollisionRepr count) */
#define OC_STAT_ERRORS 4     /* envs that hit the ERR condition */
#define OC_NSTATS 5

typedef struct oc_level_desc {
    int32_t width, height;           /* 3..255; width*height <= OC_MAX_CELLS */
    int32_t num_items;               /* <= OC_MAX_ITEMS; OC_ENC_PRESENCE: at most one of each food
                                        type, OC_ENC_COUNTS: at most OC_MC_MAX_PER_FOOD */
    int32_t num_spawns;              /* >= num_agents */
    int32_t num_goals;               /* 1..OC_MAX_GOALS Deliver goal masks */
    uint8_t tiles[OC_MAX_CELLS];     /* OC_TILE_* per cell, cell = y*width + x */
    uint16_t item_cell[OC_MAX_ITEMS]; /* initial item cells, map scan order */
    uint8_t item_mask[OC_MAX_ITEMS]; /* initial item content masks */
    uint8_t spawn_x[OC_MAX_AGENTS];
    uint8_t spawn_y[OC_MAX_AGENTS];
    uint8_t goal_mask[OC_MAX_GOALS];
    int32_t encoding;                /* OC_ENC_*: how item_mask / goal_mask (and every state's item
                                        masks and oc_subtask masks) encode contents */
} oc_level_desc;

typedef struct oc_layout {
    int64_t pitch;          /* bytes per byte-plane */
    int64_t state_bytes;    /* num_planes * pitch */
    int32_t num_agents;     /* A */
    int32_t num_items;      /* K (item slots; >= level items, extra slots dead) */
    int32_t plane_agent_x;  /* A planes, u8 */
    int32_t plane_agent_y;  /* A planes, u8 */
    int32_t plane_agent_hold; /* A planes, u8 item slot or OC_HOLD_NONE */
    int32_t plane_item_loc; /* K planes: the item cells (u8, OC_LOC_DEAD = none), or on a wide level
                               their low bytes */
    int32_t plane_item_mask;/* K planes, u8 content mask */
    int32_t plane_t;        /* u16 step counter, spans 2 planes */
    int32_t plane_flags;    /* u8 OC_FLAG_* */
    int32_t num_planes;     /* 3A + 2K + 3; wide: 3A + 3K + 3 */
    int32_t plane_item_loc_hi; /* wide levels: K planes, the item cells' high bytes (cell =
                                  lo | hi << 8, OC_LOC_DEAD16 = none); -1 on a narrow level */
    int32_t cell_bytes;     /* 1 (narrow) or 2 (wide: more than OC_MAX_NARROW_CELLS cells) */
} oc_layout;

typedef struct oc_handle oc_handle;

/* Library identity. */
int oc_abi_version(void);
const char* oc_last_error(void);

/* The message of the last failed call on handle h (the same text oc_last_error() gave the
 * calling thread then), copied NUL-terminated into buf (at most size bytes); "" when no call
 * on h has failed.  Returns the message length. */
int oc_get_last_error(const oc_handle* h, char* buf, int64_t size);

/* Static level tables + episode settings.  max_T = --max-num-timesteps (main.py:24), 0 to
 * 65,535 (the u16 step counter; round 4 refused past 32,767); 0 = no limit, where the counter
 * wraps after 65,535 steps (the reference's keeps counting; nothing else reads it).  device = HIP ordinal the handle's launches target (recorded, validated), or
 * OC_DEVICE_HOST: a host-only handle that makes no HIP call at all (no device query, no
 * device tables); only the host entry points (oc_get_layout, oc_cpu_step, oc_reachability,
 * oc_stats_size) take it, the device ones return OC_EINVAL. */
#define OC_DEVICE_HOST (-1)
int oc_create(const oc_level_desc* level, int32_t num_agents, int32_t max_T, int32_t device,
              oc_handle** out);
int oc_destroy(oc_handle* h);

/* Layout of a B-env batch for this handle. */
int oc_get_layout(const oc_handle* h, int64_t B, oc_layout* out);

/* Broadcast the level's initial state (reset(), overcooked_environment.py:201-250) to B envs. */
int oc_reset(const oc_handle* h, void* state, int64_t B, void* stream);

/* One env step for B envs (step(), overcooked_environment.py:255-306).
 *   state_in/state_out : layout buffers (may alias: in-place is allowed)
 *   actions            : u8 [A][pitch] action codes
 *   exec_actions       : u8 [A][pitch] executed (post-collision) codes = env.agent_actions
 *                        (overcooked_environment.py:770); nullable
 *   coll_mask          : u8 [pitch] colliding pairs in itertools.combinations order
 *                        (0,1),(0,2),(0,3),(1,2),(1,3),(2,3) (overcooked_environment.py:731-752); nullable
 *   stats              : u64 partial-sum buffer of oc_stats_size() bytes (zeroed by the caller
 *                        once per window); nullable
 * An env whose input flags carry OC_FLAG_DONE is reset to the level template instead of
 * stepped (next-step auto-reset; its exec actions read OC_ACT_NOOP, coll 0). */
int oc_step(const oc_handle* h, const void* state_in, void* state_out, const uint8_t* actions,
            uint8_t* exec_actions, uint8_t* coll_mask, uint64_t* stats, int64_t B, void* stream);

/* n consecutive steps in one launch, identical to n oc_step calls with ping-pong buffers
 * (state_in -> state_out after n steps).  The state stays in registers between steps, so the
 * state is read from HBM once per launch instead of once per step.
 *   actions      : n x u8 [A][pitch], step r at actions + r*A*pitch
 *   traj         : nullable; n x [num_planes][pitch]: the state after every step (traj[r] equals
 *                  the state_out of the r-th oc_step).  state_in must lie outside it; state_out
 *                  may be exactly its last state, traj + (n-1)*num_planes*pitch, which is then
 *                  written once (no second copy of the final state); any other overlap is refused
 *   exec_actions : nullable; n x u8 [A][pitch];  coll_mask : nullable; n x u8 [pitch]
 *   stats        : accumulated over the n steps (the oc_step layout, plus completion counters
 *                  after the statistics rows that must be zero when a launch with totals starts:
 *                  a zeroed buffer from the caller, which every completed launch leaves zeroed);
 *                  nullable.  Concurrent oc_step_n calls with totals (different streams) must
 *                  not share a stats buffer, and a buffer whose launch faulted must be re-zeroed
 *   totals       : nullable (needs stats); OC_NSTATS device uint64: the launch's last wave
 *                  folds the stats buffer into it, i.e. oc_stats_reduce after the steps
 *                  without a second launch (main.py's per-episode bookkeeping for the window).
 * A call longer than one launch can carry (the trajectory and action offsets of a launch stay
 * < 2 GiB, and at most 4096 steps) runs as several launches, each starting from the previous
 * one's last trajectory state; the results are the same. */
int oc_step_n(const oc_handle* h, const void* state_in, void* state_out, const uint8_t* actions, void* traj,
              uint8_t* exec_actions, uint8_t* coll_mask, uint64_t* stats, uint64_t* totals, int64_t B, int32_t n,
              void* stream);

/* The same step on the host, for a caller without a GPU (a CPU restatement behind
 * the same ABI, same layout).  step(), overcooked_environment.py:255-306, exactly as oc_step:
 * the host pass of the kernel's own SWAR step (oc_swar.h, four envs per 32-bit word, the
 * v_perm / v_bitop3 byte operations restated bit for bit), threaded over env ranges.
 *   state_in/state_out, actions, exec_actions, coll_mask : HOST buffers in the oc_step layout
 *                 (state_in may equal state_out)
 *   totals      : nullable; OC_NSTATS host uint64, the window's statistics ADDED to it
 *   nthreads    : worker threads (0 = the host's hardware threads; at least 16 Ki envs each)
 * It never touches the device; oc_step / oc_step_n never call it (no CPU fallback). */
int oc_cpu_step(const oc_handle* h, const void* state_in, void* state_out, const uint8_t* actions,
                uint8_t* exec_actions, uint8_t* coll_mask, uint64_t* totals, int64_t B, int32_t nthreads);

/* Synthetic i.i.d. uniform action codes 0..4 for B envs at step `step`:
 * code = splitmix64(seed ^ gid*0x9E3779B97F4A7C15 ^ step*0xC2B2AE3D27D4EB4F ^ agent) % 5,
 * gid = env_offset + e (global env id: identical for any GPU count). */
int oc_gen_actions(const oc_handle* h, uint8_t* actions, int64_t B, int64_t env_offset,
                   int64_t step, uint64_t seed, void* stream);

/* Order-sensitive 64-bit checksum of the state of envs [0, B) into *out (device uint64):
 *   sum_e (2e+1) * sum_p (byte_p(e) + 1) * 0x9E3779B97F4A7C15 * (2p+1)   (mod 2^64),
 * p over the byte planes (t as its low/high byte).  A size-independent parity probe for full
 * batches (compare with a host computation without copying the batch back). */
int oc_state_checksum(const oc_handle* h, const void* state, int64_t B, uint64_t* out, void* stream);

/* Statistics: size of the partial buffer for B envs, and its reduction into OC_NSTATS
 * device uint64 totals. */
int oc_stats_size(const oc_handle* h, int64_t B, int64_t* nbytes);
int oc_stats_reduce(const oc_handle* h, const uint64_t* stats, int64_t B, uint64_t* totals,
                    void* stream);

/* ---------------------------------------------------------------------------------------
 * Navigation-planner rollout: what E2E_BRTDP evaluates per (state,
 * subtask allocation, action).  Replaces, per row:
 *   _configure_planner_level, Level 0   navigation_planner/planners/e2e_brtdp.py:383-406
 *     (agents outside the subtask become collidable AgentCounters, utils/core.py:79-93,
 *      and the items they hold leave the world)
 *   get_actions / get_single_actions    e2e_brtdp.py:151-206, navigation_planner/utils.py:55-90
 *   T(state_repr, action)               e2e_brtdp.py:103-149 (interact per subtask agent in
 *                                       order, no collision pass, joint co-location assert)
 *   is_goal_state                       e2e_brtdp.py:435-566
 *   get_lower_bound_for_subtask_given_objs  gym_cooking/envs/overcooked_environment.py:480-664
 *     -> World.get_lower_bound_between(_helper), check_bound   gym_cooking/utils/world.py:115-283
 *     over the static reachability graph            world.py:67-108 (BFS table built in oc_create)
 * ------------------------------------------------------------------------------------- */
#define OC_MAX_SUBTASKS 64
#define OC_SUB_NONE 0    /* subtask None: every state is a goal state */
#define OC_SUB_CHOP 1    /* Chop(food)     gym_cooking/recipe_planner/utils.py:128 */
#define OC_SUB_MERGE 2   /* Merge(a, b)    recipe_planner/utils.py:142 */
#define OC_SUB_DELIVER 3 /* Deliver(dish)  recipe_planner/utils.py:157 */
#define OC_LEVEL0 0      /* E2E_BRTDP planner levels, oc_subtask.level */
#define OC_LEVEL1 1

/* One planner configuration (set_settings(env, subtask, subtask_agent_names)). */
typedef struct {
    int32_t kind;          /* OC_SUB_* */
    int32_t num_agents;    /* 1 or 2 (is_joint) */
    uint8_t agent[2];      /* subtask agent indices, ascending (sim_agents order) */
    uint8_t start_mask[2]; /* start_obj content mask (Chop, Deliver: [0]); Merge: start_obj[0], [1] */
    uint8_t goal_mask;     /* goal_obj content mask (navigation_planner/utils.py:181-246) */
    uint8_t goal_count;    /* cur_obj_count of _define_goal_state at set_settings */
    uint8_t level;         /* planner level (e2e_brtdp.py:383-406): OC_LEVEL0 (agents outside the
                              subtask become AgentCounters, their items leave) or OC_LEVEL1 (every
                              agent stays; none may be moved into).  oc_rollout only; the other
                              entry points take OC_LEVEL0 */
    uint8_t reserved;
} oc_subtask;

/* rollout flags (per row) */
#define OC_ROLL_LEGAL 0x01  /* the action is in get_actions(state) (joint: both single-legal and
                               is_collision all True) */
#define OC_ROLL_GOAL 0x02   /* is_goal_state(T(state, action)); 0 on OC_ROLL_ASSERT rows */
#define OC_ROLL_ASSERT 0x04 /* joint: the two agents end co-located (the reference's
                               AssertionError at e2e_brtdp.py:143; state_out still written) */
#define OC_ROLL_RAISES 0x08 /* the reference raises configuring the planner: two agents outside the
                               subtask stand on one square (World.remove of the same Floor twice,
                               gym_cooking/utils/world.py:307-315); row copied unchanged, bound 0 */
#define OC_ROLL_BADALLOC 0x80 /* alloc id >= num_subtasks: row copied unchanged, bound 0 */

/* One rollout transition per row e < B:
 *   state_in   : states in the oc_layout (real or already Level-0 states)
 *   state_out  : the Level-0 next state: agents outside the subtask keep their location with
 *                hold = OC_HOLD_NONE and their held items dead; t and flags copied
 *   actions    : u8 [A][pitch] codes; only the subtask agents' rows are read
 *   alloc      : nullable u8 [pitch] index into subtasks per row (NULL: subtasks[0])
 *   subtasks   : host array of num_subtasks (<= OC_MAX_SUBTASKS) planner configurations
 *   out_flags  : u8 [pitch] OC_ROLL_* ;  lower_bound : f32 [pitch], the lower bound of the
 *                next state before the planner's cost factor (value_init: v_l = 1.1*lb - 1.09,
 *                v_u = 6.05*lb; goal states have value 0) */
/* Level: with OC_LEVEL1 in a configuration's `level` the row keeps every agent (the planner's
 * Level-1 env, e2e_brtdp.py:383-392): nothing is removed, no agent's cell may be moved into. */
int oc_rollout(const oc_handle* h, const void* state_in, void* state_out, const uint8_t* actions,
               const uint8_t* alloc, const oc_subtask* subtasks, int32_t num_subtasks,
               uint8_t* out_flags, float* lower_bound, int64_t B, void* stream);

/* ---------------------------------------------------------------------------------------
 * Bayesian-delegation action likelihood: per row,
 *   BayesianDelegator.prob_nav_actions(obs_tm1, actions_tm1, subtask, subtask_agent_names,
 *                                      beta, no_level_1=True)
 *     gym_cooking/delegation_planner/bayesian_delegator.py:461-689
 * for a planner whose values are all value_init's (a fresh E2E_BRTDP, e2e_brtdp.py:678-729):
 *   Q(s, a) = cost(a) + v_l(T(s, a)),  cost = 1.0 + 0.1 per moving subtask agent (:816-826),
 *   v_l = 0 on goal states, else 1.1 * lower_bound - 1.09;
 *   p = softmax(beta * (Q(s, taken) - Q(s, a')))[taken] over get_actions(s) (joint actions of a
 *   pair that contains self_agent keep the other agent's taken action, :676-680);
 *   subtask None (one agent): softmax(beta * [p0, (1 - p0) / n, ...])[taken != (0,0)], n = the
 *   self agent's movable actions in the full (not Level-0) state.
 * The reference's own bayes_update runs Level 1 (other agents' planners predict their moves)
 * and BRTDP updates its values between calls; neither is restated here.
 * ------------------------------------------------------------------------------------- */
#define OC_LIK_OK 0x01       /* likelihood computed */
#define OC_LIK_RAISES 0x04   /* the reference raises: taken action not in get_actions, a joint T
                                co-location assert, two removed agents on one square (Level-0
                                configuration), or None for two agents */
#define OC_LIK_ZERODIV 0x08  /* None subtask and the self agent has no movable action */
#define OC_LIK_BADALLOC 0x80 /* alloc id >= num_subtasks */

/*   state        : obs_tm1 states (oc_layout), B rows
 *   taken        : u8 [A][pitch] executed actions actions_tm1 (env.agent_actions, :770)
 *   alloc/subtasks/num_subtasks : as oc_rollout (goal_count = the planner's cur_obj_count)
 *   self_agent   : the delegating agent's index (BayesianDelegator.agent_name)
 *   likelihood   : f64 [pitch]; out_flags : u8 [pitch] OC_LIK_* */
int oc_nav_likelihood(const oc_handle* h, const void* state, const uint8_t* taken, const uint8_t* alloc,
                      const oc_subtask* subtasks, int32_t num_subtasks, int32_t self_agent, double beta,
                      double none_action_prob, double* likelihood, uint8_t* out_flags, int64_t B, void* stream);

/* Which kernel oc_nav_likelihood runs on handle h: OC_LIK_FORM_AUTO (the default: the
 * compacted form, whose rollouts are spread over the wave, where the level's tables leave it
 * the LDS; else the grouped form) or OC_LIK_FORM_GROUPED (the grouped form always).  The two
 * give the same bits; this exists so a test can run the grouped form on any level. */
#define OC_LIK_FORM_AUTO 0
#define OC_LIK_FORM_GROUPED 1
int oc_set_likelihood_form(oc_handle* h, int32_t form);

/* The level's static reachability graph, World.make_reachability_graph (utils/world.py:67-108),
 * as built by oc_create: nodes are (cell, approach) with approach 0..3 = World.NAV_ACTIONS (the
 * side a collidable square is reached from) and 4 = (0, 0) (a Floor square).  Host data; works
 * without a device.
 *   num_nodes : out, n
 *   node_of   : nullable u16 [W*H*5]: node id of (cell, approach), 0xFFFF = not a node
 *   dist      : nullable u8 [n][n]: nx.shortest_path_length between nodes, 0xFF = no path
 * World.get_lower_bound_between(_helper) (world.py:115-283) evaluates over exactly this table.
 * The planner kernels keep the distance table in LDS for a graph of at most 360 nodes, in device
 * memory past that (a narrow level: every node its 255 cells can make; a wide one: up to 5,120).
 * A graph with a BFS distance of 255 or more (a maze kitchen's corridors) has u16 tables, in
 * device memory (ABI 10; ABI 9 refused it): oc_reachability then fails with OC_ELEVEL when
 * `dist` is given (the u8 table cannot hold it), and oc_reachability16 gives it. */
int oc_reachability(const oc_handle* h, int32_t* num_nodes, uint16_t* node_of, int64_t node_of_len, uint8_t* dist,
                    int64_t dist_len);
/* The same with u16 distances (0xFFFF = no path), for every level (ABI 10). */
int oc_reachability16(const oc_handle* h, int32_t* num_nodes, uint16_t* node_of, int64_t node_of_len, uint16_t* dist,
                      int64_t dist_len);

/* ---------------------------------------------------------------------------------------
 * Subtask bounds on full environment states (no planner Level-0 view): for every env e and
 * every configuration i of the call,
 *   lower_bound[i][e] = env.get_lower_bound_for_subtask_given_objs(subtask, agents, start_obj,
 *                        goal_obj, subtask_action_obj)
 *                       gym_cooking/envs/overcooked_environment.py:594-664, with
 *                       get_AB_locs_given_objs :480-589 and World.get_lower_bound_between(_helper)
 *                       utils/world.py:115-283 (None: perimeter + 1 + holding penalty)
 *   doable[i][e]      = BayesianDelegator.subtask_alloc_is_doable(env, subtask, agents)
 *                       delegation_planner/bayesian_delegator.py:98-156 (None: 1; else the
 *                       get_lower_bound_between distance < world.perimeter), the feasibility
 *                       test of prune_subtask_allocs (:200-260)
 * Replaces the per-(state, allocation) Python calls of the delegation planner's prior setup
 * (set_priors -> prune_subtask_allocs) and of a drop-in env's planner queries.
 *   state       : B states (oc_layout)
 *   subtasks    : host array of num_subtasks (<= OC_MAX_SUBTASKS); goal_count is ignored
 *   lower_bound : f32 [num_subtasks][pitch];  doable : u8 [num_subtasks][pitch]
 * ------------------------------------------------------------------------------------- */
int oc_subtask_bounds(const oc_handle* h, const void* state, const oc_subtask* subtasks, int32_t num_subtasks,
                      float* lower_bound, uint8_t* doable, int64_t B, void* stream);

/* ---------------------------------------------------------------------------------------
 * Image observation: what GameImage.get_image_obs returns after on_render
 *   gym_cooking/misc/game/gameimage.py:31-51, game.py:56-186
 * per env: the static level image (floor fill, counters with a 1-px border, delivery and
 * cutboard sprites; built once on the host by gym_cooking_amd/render.py), then every item
 * that is not held (tile-size sprite; a plate first, its contents at the container size /
 * offset), then each agent in order with its held item (holding size / offset), each sprite
 * blended per pixel with SDL 1.2's ALPHA_BLEND (d += ((s - d) * a + 255) >> 8, a = 0 skipped).
 * Output u8 [B][H*tile][W*tile][3]; byte c of a pixel = source channel (chan_map >> 8c) & 0xFF
 * (0 R, 1 G, 2 B, 3 constant 0).  The reference reads its 0x00RRGGBB pixels through
 * pygame.Color(int) (0xRRGGBBAA) and stores (g, b, r) = (R, G, 0): OC_CHAN_REFERENCE.
 * ------------------------------------------------------------------------------------- */
#define OC_RENDER_SIZES 4          /* tile, container, holding, holding container */
#define OC_CHAN_RGB 0x00020100u
#define OC_CHAN_REFERENCE 0x00030100u

typedef struct {
    int32_t tile;                         /* pixels per cell (Game.scale, 80; a multiple of 16) */
    int32_t size[OC_RENDER_SIZES];        /* sprite edge per size class: 80, 56, 40, 28 */
    int32_t offset[OC_RENDER_SIZES];      /* sprite origin inside its cell: 0, 12, 40, 46 */
    int32_t food_base[OC_RENDER_SIZES];   /* atlas pixel offset of food sprite 0 of each size class;
                                             food sprite i of class c at food_base[c] + i*size[c]^2 */
    int32_t plate_off[2];                 /* plate sprite at tile size, at holding size */
    int32_t agent_off[OC_MAX_AGENTS];     /* agent-<colour> sprite (utils/agent.py:25 colour order) */
    uint8_t food_sprite[128];             /* plate-less content mask -> food sprite index, 0xFF none */
    uint32_t chan_map;                    /* OC_CHAN_* */
} oc_render_desc;

/*   state      : B states (oc_layout)
 *   atlas      : device u32 RGBA sprites (R | G<<8 | B<<16 | A<<24), laid out as desc says
 *   background : device u32 RGBX [H*tile][W*tile], the static level image
 *   out        : device u8 [B][H*tile][W*tile][3] */
int oc_render(const oc_handle* h, const void* state, const uint32_t* atlas, const uint32_t* background,
              const oc_render_desc* desc, uint8_t* out, int64_t B, void* stream);

/* oc_render with the draw order of objects that share a square (Game.on_render draws the
 * objects not held in world.objects order, game.py:62-74: name groups in first-insertion
 * order, each in insertion order -- episode history, world.py:304-315, interact.py:46-52).
 *   draw_rank : device u8 [K][pitch] or NULL; objects of one square are drawn in ascending
 *               rank, ties in slot order.  NULL: slot order (oc_render).  The host side's
 *               render.DrawOrder replays the reference's order from consecutive states. */
int oc_render_ordered(const oc_handle* h, const void* state, const uint8_t* draw_rank, const uint32_t* atlas,
                      const uint32_t* background, const oc_render_desc* desc, uint8_t* out, int64_t B,
                      void* stream);

/* ---------------------------------------------------------------------------------------
 * Grid observation and legal-move masks (ABI 11): what a batched policy reads per env, at a
 * size a step can afford (a 7x7 kitchen with two agents: 588 B in u8; the image is 940,800 B).
 *
 * obs[e][c][y][x], C = OC_OBS_CHANNELS(A) planes of H x W small counts, a pure function of env
 * e's state and the level:
 *   0, 1, 2   Counter, Cutboard, Delivery: 1 on squares of that class (the GridSquare subclasses
 *             in world.objects, gym_cooking/utils/core.py:28-120); Floor is all-zero
 *   3, 4      FreshTomato, ChoppedTomato: for every Object in world.objects, held or not, at
 *   5, 6      FreshLettuce, ChoppedLettuce   obj.location (a held object carries its holder's
 *   7, 8      FreshOnion, ChoppedOnion       location): +1 per content of that food in that
 *   9         Plate                          state / per Plate content (core.py:130-305)
 *   10 + i    agent i: 1 at sim_agents[i].location
 * Dead item slots contribute nothing; several objects on one square add up (delivered dishes;
 * two tomatoes in one dish of an OC_ENC_COUNTS level give 2); both content encodings decode to
 * the same channels (OC_ENC_COUNTS: OC_MC_FRESH marks a single fresh food, every other food is
 * chopped).  t and the flags are not encoded (the caller has their planes); DONE and ERR envs
 * are encoded as their stored state is.
 *   view_agent : -1: agent channels in index order; a in [0, A): agent i is channel
 *                10 + ((i - a) mod A), so the viewing agent is always channel 10
 *
 * action_mask[a][e], u8: bit k (k = 0..3) is set iff World.NAV_ACTIONS[k] is in
 * get_single_actions(env, sim_agents[a]) (gym_cooking/navigation_planner/utils.py:55-90) on the
 * full env: every agent present, no agent's square may be entered (the agent's own included,
 * which matters where World.inbounds, utils/world.py:432-436, clamps an off-grid target onto
 * it), Floor and Delivery are open, a Counter or Cutboard is legal as a put-down, a pick-up
 * or a merge (core.mergeable, core.py:222-241).  Bit OC_ACT_NOOP is always set.
 * ------------------------------------------------------------------------------------- */
#define OC_OBS_STATIC 3
#define OC_OBS_ITEM 7
#define OC_OBS_CHANNELS(A) (OC_OBS_STATIC + OC_OBS_ITEM + (A))
#define OC_OBS_U8 0
#define OC_OBS_F16 1

/*   state       : B states (oc_layout), device memory
 *   obs         : nullable; device [B][C][H][W], contiguous, env-major (torch NCHW), u8
 *                 (OC_OBS_U8) or IEEE half (OC_OBS_F16; the counts are exact).  Exactly B*C*H*W
 *                 elements are written, not one byte past them; any element-aligned address
 *                 (16-byte alignment keeps every store full width); more than 4 GiB is fine
 *   action_mask : nullable; device u8 [A][pitch].  Columns past B as exec_actions: the batch's
 *                 last 4-env word may be completed (no-op only), nothing at or past the next
 *                 multiple of 4 above B is written
 *   dtype       : OC_OBS_U8 or OC_OBS_F16;  view_agent : -1 or 0..A-1
 * Both outputs NULL, another dtype or view_agent is OC_EINVAL.  Stream-ordered, no allocation,
 * no synchronisation (hipGraph-capturable, as oc_step); one launch for both outputs. */
int oc_observe(const oc_handle* h, const void* state, void* obs, uint8_t* action_mask,
               int32_t dtype, int32_t view_agent, int64_t B, void* stream);

/* The same on the host (what oc_cpu_step is to oc_step): HOST buffers, works on OC_DEVICE_HOST
 * handles, the kernel's decode compiled for the host, threaded over env ranges (nthreads 0 = the
 * host's hardware threads; at least 16 Ki envs each).  Columns of action_mask past B are not
 * written.  It never touches the device; oc_observe never calls it. */
int oc_cpu_observe(const oc_handle* h, const void* state, void* obs, uint8_t* action_mask,
                   int32_t dtype, int32_t view_agent, int64_t B, int32_t nthreads);

/* ---------------------------------------------------------------------------------------
 * Subtask progress (ABI 12): per env and per subtask the reference agent's goal-object count,
 * the completion events of a transition and a shaped reward.  A trainer's dense signal, a
 * delegator's incomplete_subtasks test, the goal_count of an oc_rollout configuration.
 *
 * Of a subtask only `kind` and `goal_mask` are read (the other fields are ignored, as
 * oc_subtask_bounds ignores goal_count).  count_i(s), u8, of a state s:
 *   A slot is live when its cell is not OC_LOC_DEAD / OC_LOC_DEAD16.  Its cell is the item's
 *   cell; for a held item (a live slot some agent's hold plane names; the lowest such agent)
 *   that is its holder's square y * W + x, as the reference's held object carries its holder's
 *   location (SimAgent.acquire / move_to, utils/agent.py:408-423).  States the engine or the
 *   oracle made keep the item cell on the holder already; the count does not rely on it.
 *   OC_SUB_CHOP, OC_SUB_MERGE : the number of distinct cells of live slots whose mask byte equals
 *       goal_mask = len(world.get_all_object_locs(goal_obj)), a list(set(...)) of locations
 *       (utils/world.py:354-387; agent.py:286-353), in either mask encoding (byte equality)
 *   OC_SUB_DELIVER : the number of live slots, not held, with mask == goal_mask on any Delivery
 *       square: the reference takes a list here, not a set (agent.py:354-361), so two equal
 *       dishes on one Delivery square count twice
 *   OC_SUB_NONE : 0
 * Per step r of a call, prev = states[r-1] (state_prev for r = 0), cur = states[r]:
 *   counts[r][i][e] = count_i(cur)
 *   event i         = prev does not carry OC_FLAG_DONE and count_i(cur) > count_i(prev): exactly
 *       is_subtask_complete(cur.world) (agent.py:363-368) of an agent whose
 *       def_subtask_completion ran on prev.  An env that was DONE at prev is the auto-reset
 *       template in cur and reports no event (build-defined, like auto-reset itself); a step that
 *       ends in ERR leaves the state unchanged and so reports none; the delivering step that
 *       sets DONE and SUCCESS does report its Deliver event.
 *   events[r][c][e], u8 : bit b of plane c is subtask 8c + b; OC_PROGRESS_EVENT_PLANES(n) planes
 *   reward[r][e], f32   : from +0.0f, + weights[i] for every set event in ascending i, plain f32
 *       adds in that order (weights NULL: all 1.0f, the number of events)
 * ------------------------------------------------------------------------------------- */
#define OC_PROGRESS_EVENT_PLANES(n) (((n) + 7) / 8)

/*   state_prev : the state before states[0] (oc_layout), device memory
 *   states     : n >= 1 consecutive layout buffers, state_bytes apart: one state (n = 1), or an
 *                oc_step_n trajectory with state_prev the launch's state_in
 *   subtasks   : host array of num_subtasks (1..OC_MAX_SUBTASKS); kinds OC_SUB_*
 *   weights    : host array of num_subtasks floats, or NULL (all 1.0f)
 *   counts     : nullable; n x u8 [num_subtasks][pitch]
 *   events     : nullable; n x u8 [OC_PROGRESS_EVENT_PLANES(num_subtasks)][pitch]
 *   reward     : nullable; n x f32 [pitch], 16-byte aligned
 * Inputs are read-only and may alias each other (state_prev == states: no events, valid counts).
 * Columns past B as exec_actions: the batch's last 4-env word may be completed with zeros (for
 * reward the floats up to the next multiple of 4 above B); nothing at or past that is written.
 * A bad n, num_subtasks or kind, all three outputs NULL, or a host-only handle is OC_EINVAL.
 * Stream-ordered, no allocation, no synchronisation (hipGraph-capturable, as oc_step).  One
 * launch whatever n: every offset inside it is 64-bit, and each state is loaded once (step r's
 * cur is step r + 1's prev). */
int oc_progress(const oc_handle* h, const void* state_prev, const void* states, int32_t n,
                const oc_subtask* subtasks, int32_t num_subtasks, const float* weights,
                uint8_t* counts, uint8_t* events, float* reward, int64_t B, void* stream);

/* The same on the host (what oc_cpu_step is to oc_step): HOST buffers, works on OC_DEVICE_HOST
 * handles, the kernel's count and event functions compiled for the host, threaded over env
 * ranges (nthreads 0 = the host's hardware threads; at least 16 Ki envs each).  Nothing past
 * column B is written.  It never touches the device; oc_progress never calls it. */
int oc_cpu_progress(const oc_handle* h, const void* state_prev, const void* states, int32_t n,
                    const oc_subtask* subtasks, int32_t num_subtasks, const float* weights,
                    uint8_t* counts, uint8_t* events, float* reward, int64_t B, int32_t nthreads);

/* ---------------------------------------------------------------------------------------
 * Randomised episode starts (additive to ABI 12): per env, the agents on other Floor squares and
 * the level's items on other Counter squares.  The reference has no batch and no randomisation, so
 * the surface is build-defined like auto-reset; a drawn start is exactly the state the reference
 * builds when it loads the level file with its item letters and spawn lines moved to the drawn
 * cells: load_level (gym_cooking/envs/overcooked_environment.py:144-193) makes one object per map
 * letter on a Counter (:158-165) and one agent per spawn line (:186-193).
 *
 * The start distribution of a handle: per agent i a list LA_i of Floor cells and one list LI of
 * item cells, both in ascending cell id.  Defaults, from the level:
 *   LA_i : the Floor cells 4-connected through Floor to spawn i (a full divider keeps each agent
 *          on its own side)
 *   LI   : the cells of class OC_TILE_COUNTER (not Cutboard, not Delivery) with at least one
 *          Floor 4-neighbour.  The template may keep an item on a counter outside LI: the
 *          template is not a draw.
 * The draw of env e, global id gid = env_offset + e (identical for any split of the envs over
 * GPUs, as oc_gen_actions):
 *   base    = seed ^ gid * 0x9E3779B97F4A7C15 ^ round * 0xC2B2AE3D27D4EB4F
 *   u(d)    = splitmix64(base ^ (0x53540000 + d))        (oc_gen_actions' splitmix64; the offset
 *                                                         keeps the two streams apart)
 *   r(d, n) = (uint32)(((u(d) >> 32) * n) >> 32)
 *   agents i = 0..A-1 : with m = the earlier agents standing on a cell of LA_i, agent i takes the
 *             r(i, |LA_i| - m)-th cell of LA_i, ascending, that no earlier agent occupies;
 *             hold = OC_HOLD_NONE
 *   items, live template slots k ascending : with j = the earlier live slots, slot k takes the
 *             r(16 + k, |LI| - j)-th cell of LI, ascending, not taken by an earlier slot, and
 *             keeps the template's mask byte; dead slots stay dead
 *   t = 0, flags = 0.  A part `what` does not select keeps the template's values.
 * Every draw is exact and bounded: no rejection loop, no fallback.
 * ------------------------------------------------------------------------------------- */
#define OC_START_AGENTS 1
#define OC_START_ITEMS 2

/* Set the handle's start distribution (what a caller of load_level chooses by editing the level
 * file, overcooked_environment.py:144-193):
 *   agent_ok : u8 [A][W*H], non-zero = agent i may start on the cell; NULL = the default lists
 *   item_ok  : u8 [W*H], non-zero = an item may start on the cell; NULL = the default list
 * Refused with a message, the handle unchanged: a non-Floor cell in agent_ok or a cell in item_ok
 * that is not class Counter (OC_EINVAL), fewer than A cells in an agent's list or fewer item cells
 * than the level has items (OC_EINVAL; OC_ELEVEL when it is the level's default list that is too
 * short).  Host masks; may allocate and copy as oc_create does, is not stream-ordered (calls in
 * flight on the handle must have completed), and works on OC_DEVICE_HOST handles. */
int oc_set_start_cells(oc_handle* h, const uint8_t* agent_ok, const uint8_t* item_ok);

/* The effective masks (defaults included) as 0 / 1 bytes: agent_ok u8 [A][W*H], item_ok u8 [W*H];
 * either may be NULL. */
int oc_get_start_cells(const oc_handle* h, uint8_t* agent_ok, uint8_t* item_ok);

/* reset() (overcooked_environment.py:201-250) of the level file with moved letters and spawn lines,
 * per env (the draw above).
 *   state      : B states (oc_layout), device memory, 8-byte aligned
 *   state_prev : NULL: every env below B gets a fresh start (reset()).  Else only the envs whose
 *                state_prev flags carry OC_FLAG_DONE are written and every other byte of `state` is
 *                left as it is: called after oc_step(state_prev -> state) it replaces exactly the
 *                envs the step just auto-reset to the template (auto-reset's timing, t = 0 and
 *                no-op executed actions, is unchanged).  state_prev == state restarts the DONE envs
 *                in place (each word's flags are read before it is written).
 *   env_offset : global id of env 0 (>= 0);  seed, round : the draw's;  what : OC_START_* bits
 * Columns past B: with state_prev NULL the batch's last 4-env word may be completed with the
 * template; nothing at or past the next multiple of 4 above B is written (unlike oc_reset, which
 * fills the pitch: a buffer that has never been reset keeps whatever bytes it had in those columns,
 * which the step kernels step but no output or statistic counts).  what = 0 or other bits,
 * or a host-only handle, is OC_EINVAL; a level whose default lists are too short for it and that has
 * no lists set is OC_ELEVEL.  Stream-ordered, no allocation, no synchronisation
 * (hipGraph-capturable, as oc_step).  oc_step_n keeps template restarts inside a launch: its
 * trajectories never hold a drawn start. */
int oc_reset_random(const oc_handle* h, void* state, const void* state_prev, int64_t B, int64_t env_offset,
                    uint64_t seed, uint64_t round, int32_t what, void* stream);

/* The same on the host (what oc_cpu_step is to oc_step): HOST buffers, works on OC_DEVICE_HOST
 * handles, the kernel's draw functions compiled for the host, threaded over word ranges (nthreads
 * 0 = the host's hardware threads; at least 16 Ki envs each).  Nothing past column B is read or
 * written.  It never touches the device; oc_reset_random never calls it. */
int oc_cpu_reset_random(const oc_handle* h, void* state, const void* state_prev, int64_t B, int64_t env_offset,
                        uint64_t seed, uint64_t round, int32_t what, int32_t nthreads);

/* ---------------------------------------------------------------------------------------
 * Subtask-following actions (additive to ABI 12): the generative side of oc_nav_likelihood's
 * agent model, for a scripted partner.  Per row, the whole Boltzmann distribution over
 * get_actions(s) under the row's planner configuration, and one action taken from it:
 *   p(a | s, subtask) ~ exp(-beta * Q(s, a)),  Q as oc_nav_likelihood's (a fresh planner's
 *   value_init values; bayesian_delegator.py:461-689, e2e_brtdp.py:678-760).
 * Candidate k is a0 for a one-agent configuration and a0 * 5 + a1 for two agents (the
 * likelihood's order); it is legal iff the action is in get_actions on the row's Level-0 view.
 * There is no self agent and no taken action: a joint configuration gets the full 25-way
 * distribution.  For a subtask row that does not raise, in f64:
 *   m = min of Q_k over the legal k;  w_k = exp(beta * (m - Q_k));
 *   S = the w_k of the legal k added in ascending k, starting from +0.0;
 *   p_k = w_k / S;  illegal candidates have p_k = +0.0.
 * OC_SUB_NONE with one agent a: the likelihood's closed form with a as both the self agent and
 * the acting agent: n = a's movable actions in the full state, x0 = beta * nap,
 * x1 = beta * ((1 - nap) / n), mm = max(x0, x1), S = exp(x0 - mm) then n adds of exp(x1 - mm),
 * p(no-op) = exp(x0 - mm) / S, p of each movable action = exp(x1 - mm) / S; n = 0: p(no-op) = 1.0
 * and the row is OK.
 * mode bit 1, the count is_goal_state compares with: OC_POLICY_COUNT_TABLE the configuration's
 * goal_count; OC_POLICY_COUNT_STATE the number of goal objects in the row's own Level-0 view, the
 * cur_obj_count a planner gets from _define_goal_state when set_settings runs on this very state
 * (e2e_brtdp.py:435-566): a partner that was "configured now", right for a batch whose envs are
 * at different points of a recipe.
 * mode bit 0, the choice: OC_POLICY_GREEDY the lowest legal k with Q_k == m (None: the no-op if
 * x0 >= x1 or n = 0, else the lowest movable action).  OC_POLICY_SAMPLE one number per row:
 *   key = seed ^ gid * 0x9E3779B97F4A7C15 ^ step * 0xC2B2AE3D27D4EB4F ^ (0x504F4C00 + agent[0]),
 *   gid = env_offset + e (identical for any split of the envs over GPUs, as oc_gen_actions),
 *   u = (splitmix64(key) >> 11) * 2^-53;  c = +0.0; for k = 0 .. ncand - 1 ascending (ncand = 5
 *   or 25, the row's own): c += p_k, the first k with u < c is taken; if rounding leaves none,
 *   the highest legal k.  The draw is defined on the p values the call returns: a caller can
 *   replay it exactly from `probs`.
 * ------------------------------------------------------------------------------------- */
#define OC_POL_OK 0x01        /* distribution computed, action written */
#define OC_POL_RAISES 0x04    /* the reference raises: two removed agents on one square (Level-0
                                 configuration), a legal joint candidate whose T ends co-located,
                                 None for two agents, or no legal candidate */
#define OC_POL_BADALLOC 0x80  /* alloc id >= num_subtasks */
#define OC_POLICY_SAMPLE 0      /* mode bit 0 */
#define OC_POLICY_GREEDY 1
#define OC_POLICY_COUNT_TABLE 0 /* mode bit 1: goal test against the table's goal_count */
#define OC_POLICY_COUNT_STATE 2 /* ... against the row's own count */

/*   state, alloc, subtasks, num_subtasks, beta, none_action_prob : as oc_nav_likelihood
 *                (OC_LEVEL0 configurations only; alloc NULL: subtasks[0])
 *   env_offset, step (>= 0), seed : the draw's
 *   actions    : u8 [A][pitch], required.  Only the bytes of row e's subtask agents are written,
 *                with the chosen a0 / a1 (OC_ACT_NOOP on OC_POL_RAISES rows, nothing on
 *                OC_POL_BADALLOC rows); every other agent's byte and every column >= B stays
 *                untouched, so a learner's actions in the same buffer survive
 *   probs      : nullable; f64 [num_cand][pitch], 8-byte aligned, plane k = p_k.  num_cand is 5
 *                or 25; 5 with a two-agent configuration in the table is OC_EINVAL.  A one-agent
 *                row of a 25-candidate call fills planes 0..4 and zeroes the rest; rows that are
 *                not OK are all zero; columns >= B are untouched
 *   out_flags  : u8 [pitch] OC_POL_*, required; columns >= B untouched
 * Stream-ordered, no allocation, no synchronisation (hipGraph-capturable, as oc_step).  Bad
 * arguments and host-only handles are OC_EINVAL. */
int oc_nav_policy(const oc_handle* h, const void* state, const uint8_t* alloc, const oc_subtask* subtasks,
                  int32_t num_subtasks, double beta, double none_action_prob, int32_t mode, int64_t env_offset,
                  int64_t step, uint64_t seed, uint8_t* actions, double* probs, int32_t num_cand,
                  uint8_t* out_flags, int64_t B, void* stream);

/* The same on the host (what oc_cpu_step is to oc_step): HOST buffers, works on OC_DEVICE_HOST
 * handles, the kernel's row functions compiled for the host, threaded over env ranges (nthreads
 * 0 = the host's hardware threads; at least 1,024 rows each).  Nothing past column B is
 * written.  It never touches the device; oc_nav_policy never calls it.  The two agree on flags
 * and, up to the last bits of exp and of a fused multiply-add, on probs. */
int oc_cpu_nav_policy(const oc_handle* h, const void* state, const uint8_t* alloc, const oc_subtask* subtasks,
                      int32_t num_subtasks, double beta, double none_action_prob, int32_t mode, int64_t env_offset,
                      int64_t step, uint64_t seed, uint8_t* actions, double* probs, int32_t num_cand,
                      uint8_t* out_flags, int64_t B, int32_t nthreads);

/* ---------------------------------------------------------------------------------------
 * Per-env subtask choice for scripted agents (additive to ABI 12): the byte oc_nav_policy's
 * `alloc` takes, made on the device.  Per env and scripted agent, the reference agent's subtask
 * bookkeeping and a greedy delegator's choice over the pruned hypothesis space:
 *   refresh_subtasks, def_subtask_completion, is_subtask_complete
 *                                   gym_cooking/utils/agent.py:151-171, 286-368
 *   add_greedy_subtasks             delegation_planner/bayesian_delegator.py:892-923
 *   prune_subtask_allocs            bayesian_delegator.py:200-256
 *   subtask_alloc_is_doable         bayesian_delegator.py:98-156
 *   add_dc_subtasks (no two agents on one subtask: OC_TASK_DISTINCT)   bayesian_delegator.py:928-1000
 * Build-defined, like auto-reset, oc_reset_random and oc_nav_policy's fresh-planner Q: only the
 * ranking is this build's, the smallest get_lower_bound_for_subtask_given_objs, which orders the
 * candidates as 1 / (1.1 * lb - 1.09) does wherever that is positive.  It is not set_priors: the
 * reference ranks allocations by 1 / v_l read after a BRTDP search (bayesian_delegator.py:162-194,
 * 296-369), and its Bayesian updates over time are not restated either.
 *
 * The rule, for env e and the scripted agents m = 0 .. M-1 in the caller's order, a = agents[m]:
 *   1. initialise, if the env is selected for it: incomplete = all S bits, cur = S, cnt = 0
 *   2. refresh (agent.py:151-171): if cur < S and count_cur(state) > cnt: clear bit cur, cur = S,
 *      OC_TASKF_COMPLETED.  count_i is oc_progress's count_i
 *   3. candidates C: every i < S with bit i set, kind != OC_SUB_NONE and doable_i; with
 *      OC_TASK_DISTINCT also i != the cur of every scripted agent m' < m as its step 4 of this call
 *      left it.  doable_i and lb_i are what oc_subtask_bounds gives on this state for the row
 *      {kind, num_agents 1, agent {a}, start_mask, goal_mask}
 *   4. choose: with OC_TASK_COMMIT, cur < S and cur in C: keep cur.  Otherwise new = the i in C
 *      with the smallest lb_i (f32 <, ties to the lowest i), or S when C is empty; if new != cur and
 *      new < S: cnt = count_new(state); cur = new.  OC_TASKF_SWITCHED iff cur at exit differs from
 *      cur at entry (the value after step 1)
 * ------------------------------------------------------------------------------------- */
#define OC_TASK_INIT     1   /* every env below B starts its episode: task state initialised first */
#define OC_TASK_COMMIT   2   /* keep the current subtask while it is still a candidate */
#define OC_TASK_DISTINCT 4   /* a subtask an earlier scripted agent holds after its own choice in this
                                call is no candidate */
#define OC_TASKF_COMPLETED 0x01  /* the current subtask's count rose: removed from the incomplete set */
#define OC_TASKF_SWITCHED  0x02  /* cur at exit != cur at entry (entry = after initialisation) */
#define OC_TASKF_REINIT    0x04  /* task state initialised in this call */
#define OC_TASK_PLANES(S) (OC_PROGRESS_EVENT_PLANES(S) + 2)

/*   state        : B states (oc_layout); DONE and ERR envs are processed as their stored state is
 *   state_prev   : nullable.  The envs whose state_prev flags carry OC_FLAG_DONE are the ones the
 *                  step that produced `state` auto-reset: their task state is initialised first
 *                  (OC_TASKF_REINIT; oc_reset_random's convention).  OC_TASK_INIT initialises every
 *                  env and wins over state_prev; with neither, nothing is initialised
 *   subtasks     : host array of S = num_subtasks rows; only kind, start_mask and goal_mask are read
 *                  (capi.progress_subtasks rows serve).  OC_SUB_NONE rows are never candidates
 *   agents       : host array of M = num_scripted distinct agent indices, in the caller's order: the
 *                  priority order of OC_TASK_DISTINCT
 *                  1 <= M <= A, 1 <= S <= 63 (index S is the None row of a policy table),
 *                  M * S <= OC_MAX_SUBTASKS (the staging of the planner tables)
 *   tstate       : required, caller-owned, u8 [M][OC_TASK_PLANES(S)][pitch], read and written in
 *                  place (each env's bytes are read before they are written).  With EP =
 *                  OC_PROGRESS_EVENT_PLANES(S), the planes of scripted agent m:
 *                    0 .. EP-1 : the incomplete set, bit b of plane c is subtask 8c + b (oc_progress's
 *                                events numbering); bits >= S are zero
 *                    EP        : cur, the subtask the agent follows, or S for None: oc_nav_policy's
 *                                `alloc` for a table whose rows 0 .. S-1 are these subtasks for agent m
 *                                and whose row S is None (capi.policy_subtasks(subtasks + [None], ..))
 *                    EP + 1    : cnt, the goal-object count of cur when it was taken
 *   bound        : nullable, f32 [M][pitch], 4-byte aligned: the chosen subtask's lower bound, +0.0f
 *                  for None
 *   info         : nullable, u8 [M][pitch], OC_TASKF_* bits
 * Columns >= B of every buffer stay untouched.  Stream-ordered, no allocation, no synchronisation
 * (hipGraph-capturable, as oc_step).  A bad M, S, agents or flags, a NULL state, subtasks, agents
 * or tstate, a misaligned bound, or a host-only handle is OC_EINVAL; B = 0 is OK. */
int oc_task_select(const oc_handle* h, const void* state, const void* state_prev, const oc_subtask* subtasks,
                   int32_t num_subtasks, const uint8_t* agents, int32_t num_scripted, int32_t flags, uint8_t* tstate,
                   float* bound, uint8_t* info, int64_t B, void* stream);

/* The same on the host (what oc_cpu_step is to oc_step): HOST buffers, works on OC_DEVICE_HOST
 * handles, the kernel's row function compiled for the host, threaded over env ranges (nthreads
 * 0 = the host's hardware threads; at least 1,024 rows each).  It never touches the device;
 * oc_task_select never calls it.  The two agree byte for byte. */
int oc_cpu_task_select(const oc_handle* h, const void* state, const void* state_prev, const oc_subtask* subtasks,
                       int32_t num_subtasks, const uint8_t* agents, int32_t num_scripted, int32_t flags,
                       uint8_t* tstate, float* bound, uint8_t* info, int64_t B, int32_t nthreads);

/* ---------------------------------------------------------------------------------------
 * Joint and split subtask choice for one pair of scripted agents (additive to ABI 12): the three
 * bytes three oc_nav_policy launches take as `alloc`, made on the device.  oc_task_select reasons
 * about "agent a alone follows subtask i"; this call also weighs "both agents follow subtask i",
 * which is what a kitchen needs whose every subtask takes two agents (full-divider_*: an item is
 * handed over a counter wall).  Per env, the allocation space of two agents and its pruning:
 *   add_subtasks, get_other_subtask_allocations   delegation_planner/bayesian_delegator.py:697-886
 *       cooperative (t, (a0, a1)), and divide-and-conquer (t0, (a0,)), (t1, (a1,)) with t0 != t1;
 *       None is allowed for one member and not for both
 *   prune_subtask_allocs                          bayesian_delegator.py:200-256
 *   subtask_alloc_is_doable                       bayesian_delegator.py:98-156
 *   get_spatial_priors                            bayesian_delegator.py:296-369
 *       the weight of an allocation is the sum over its non-None members of
 *       1 / get_lower_bound_for_subtask_alloc
 *   refresh_subtasks                              gym_cooking/utils/agent.py:151-171
 * Build-defined, like oc_task_select: the argmax of the spatial prior in place of BRTDP-valued
 * priors and Bayesian updates over time, one incomplete set shared by the pair, and the tie rules.
 *
 * The team is a0 = agents[0] < a1 = agents[1].  With S = num_subtasks and EP =
 * OC_PROGRESS_EVENT_PLANES(S), the team state of an env is u8 [OC_TEAM_PLANES(S) = EP + 5][pitch]:
 *   0 .. EP-1 : the incomplete set, bit b of plane c is subtask 8c + b (oc_progress's events
 *               numbering); bits >= S are zero
 *   EP        : cur0    EP + 1 : cur1    EP + 2 : curJ    EP + 3 : cnt0    EP + 4 : cnt1
 * The allocation is joint iff curJ < S; then cur0 = cur1 = OC_TEAM_OUT.  Otherwise it is split:
 * cur0 and cur1 are in [0, S], S meaning None, and curJ = OC_TEAM_OUT.  Idle is the split (S, S).
 * The three cur planes are directly the `alloc` planes of three oc_nav_policy launches: plane cur0
 * for a0's one-agent table (rows 0 .. S-1 these subtasks, row S None), plane cur1 for a1's, plane
 * curJ for the two-agent table of S rows.  oc_nav_policy flags an alloc >= its table size
 * OC_POL_BADALLOC and writes nothing for that row: "this env is not this launch's".
 *
 * The rule, for env e (count_i is oc_progress's count_i on `state`):
 *   1. initialise, if the env is selected for it: incomplete = all S bits, cur0 = cur1 = S, curJ =
 *      OC_TEAM_OUT, cnt0 = cnt1 = 0.  OC_TEAMF_REINIT
 *   2. refresh.  Joint: if count_curJ > cnt0, clear bit curJ, OC_TEAMF_COMPLETED0 | COMPLETED1.
 *      Split: for m = 0, 1: if cur_m < S and count_cur_m > cnt_m, clear bit cur_m,
 *      OC_TEAMF_COMPLETED_m.  If anything completed the allocation is dropped (cur0 = cur1 = S,
 *      curJ = OC_TEAM_OUT) and step 4 cannot keep it
 *   3. candidates, over every i < S with bit i set and kind != OC_SUB_NONE:
 *        C0: the row {kind_i, 1 agent {a0}, masks_i} is doable;  C1: the same for a1;
 *        CJ: the row {kind_i, 2 agents {a0, a1}, masks_i} is doable
 *      doable and lb are exactly oc_subtask_bounds' outputs on `state`.  The weights are f64,
 *      w = 1.0 / (double)lb (lb >= 1, world.py:264); None weighs +0.0
 *   4. keep, with OC_TEAM_COMMIT when step 2 dropped nothing.  Joint: curJ in CJ.  Split: cur0 < S,
 *      cur1 < S, cur0 in C0 and cur1 in C1 (an allocation with a None member is never kept).  Then
 *      the allocation and the counts stay; go to 7
 *   5. picks.  first_m = the i in C_m of largest w, ties to the lowest i, or S when C_m is empty;
 *      second_m = the same over C_m without first_m.  The split pick is (first_0, first_1) if they
 *      differ, and there is none if both are S.  Otherwise both name one subtask: with
 *      x = w0[first_0] + w1[second_1] and y = w0[second_0] + w1[first_1] it is (first_0, second_1)
 *      if x >= y, else (second_0, first_1).  wS = the pick's sum (one f64 add).  This is the argmax
 *      of w0_i + w1_j over all admissible (i, j), i != j: IEEE addition is monotone in each operand,
 *      so the rounded sum of the two largest terms is no smaller than any other rounded sum.
 *      The joint pick iJ = the i in CJ of largest wJ, ties to the lowest i
 *   6. choose.  The split pick is "full" when both members are < S.
 *        with OC_TEAM_SPLIT_FIRST and a full split pick: split
 *        otherwise, if CJ is non-empty and (there is no split pick or wJ[iJ] >= wS): joint
 *          (cooperative allocations come first in add_subtasks' enumeration)
 *        otherwise, if there is a split pick: split
 *        otherwise idle, OC_TEAMF_IDLE
 *   7. if (cur0, cur1, curJ) differs from its value after step 1: OC_TEAMF_SWITCHED, cnt0 = the
 *      count of a0's member on `state` (joint: of curJ; None: 0) and cnt1 = the count of a1's
 *      member (joint or None: 0).  OC_TEAMF_JOINT iff the allocation is joint at exit
 * ------------------------------------------------------------------------------------- */
#define OC_TEAM_INIT        1   /* every env below B starts its episode: team state initialised first */
#define OC_TEAM_COMMIT      2   /* keep the current allocation while all its members are candidates */
#define OC_TEAM_SPLIT_FIRST 4   /* a full split pick wins over the joint pick whatever their weights */
#define OC_TEAMF_COMPLETED0 0x01  /* a0's member's count rose: removed from the incomplete set */
#define OC_TEAMF_COMPLETED1 0x02  /* a1's member's count rose (a joint completion sets both) */
#define OC_TEAMF_SWITCHED   0x04  /* the allocation at exit differs from the one at entry (after step 1) */
#define OC_TEAMF_REINIT     0x08  /* team state initialised in this call */
#define OC_TEAMF_JOINT      0x10  /* the allocation at exit is joint */
#define OC_TEAMF_IDLE       0x20  /* step 6 found neither a split nor a joint pick */
#define OC_TEAM_OUT 0xFF          /* a cur plane's byte where the env is not that plane's launch's */
#define OC_TEAM_MAX_SUBTASKS 21   /* 3 configurations per subtask in the OC_MAX_SUBTASKS staging */
#define OC_TEAM_PLANES(S) (OC_PROGRESS_EVENT_PLANES(S) + 5)

/*   state, state_prev : as oc_task_select (OC_TEAM_INIT wins over state_prev; with neither, nothing
 *                  is initialised)
 *   subtasks     : host array of S rows, 1 <= S <= OC_TEAM_MAX_SUBTASKS; only kind, start_mask and
 *                  goal_mask are read.  OC_SUB_NONE rows are never candidates
 *   agents       : host array of 2 agent indices, a0 < a1 < A (so A >= 2)
 *   tstate       : required, caller-owned, u8 [OC_TEAM_PLANES(S)][pitch], read and written in place
 *                  (an env's bytes are read before they are written)
 *   bound        : nullable, f32 [2][pitch], 4-byte aligned: each agent's member's lower bound; the
 *                  joint bound in both planes for a joint allocation; +0.0f for None
 *   info         : nullable, u8 [pitch], OC_TEAMF_* bits
 * Columns >= B of every buffer stay untouched.  Stream-ordered, no allocation, no synchronisation
 * (hipGraph-capturable, as oc_step).  A bad S, agents or flags, A = 1, a NULL state, subtasks,
 * agents or tstate, a misaligned bound, or a host-only handle is OC_EINVAL; B = 0 is OK. */
int oc_team_select(const oc_handle* h, const void* state, const void* state_prev, const oc_subtask* subtasks,
                   int32_t num_subtasks, const uint8_t* agents, int32_t flags, uint8_t* tstate, float* bound,
                   uint8_t* info, int64_t B, void* stream);

/* The same on the host (what oc_cpu_step is to oc_step): HOST buffers, works on OC_DEVICE_HOST
 * handles, the kernel's row function compiled for the host, threaded over env ranges (nthreads
 * 0 = the host's hardware threads; at least 1,024 rows each).  It never touches the device;
 * oc_team_select never calls it.  The two agree byte for byte on tstate, bound and info (the f64
 * division and the one add are IEEE on both sides). */
int oc_cpu_team_select(const oc_handle* h, const void* state, const void* state_prev, const oc_subtask* subtasks,
                       int32_t num_subtasks, const uint8_t* agents, int32_t flags, uint8_t* tstate, float* bound,
                       uint8_t* info, int64_t B, int32_t nthreads);

/* ---------------------------------------------------------------------------------------
 * Per-env Bayesian belief over a watched agent's subtask (additive to ABI 12): Bayesian Delegation's
 * inference step on the batch.  Per env and watched agent a, a posterior over S + 1 hypotheses:
 * hypothesis i < S is "a alone follows subtasks[i]", hypothesis S is "a follows None".
 *   update_subtasks (set_priors in place of bayes_update after a completion)
 *                                   gym_cooking/utils/agent.py:176-203
 *   bayes_update                    delegation_planner/bayesian_delegator.py:1026-1072
 *   subtask_alloc_is_doable         bayesian_delegator.py:98-156
 *   prob_nav_actions (no_level_1)   bayesian_delegator.py:461-689 (the assert at :672)
 *   SubtaskAllocDistribution.__init__, delete, update, normalize, get_max
 *                                   delegation_planner/utils.py:160-215 (normalize :186-193)
 * Build-defined, like oc_task_select: one-agent hypotheses about one agent, uniform priors only
 * (the reference enumerates joint allocations and offers spatial priors), fresh-planner Q values
 * (oc_nav_policy's), and ties of the maximum go to the lowest index (get_max draws at random).
 *
 * With HP = OC_BELIEF_PLANES(S) = ceil((S + 1) / 8), the state of a watched agent is two bit sets
 * over the hypotheses, bit b of plane c being hypothesis 8c + b, bits > S zero:
 *   open : the subtasks nobody has completed this episode (and bit S)
 *   live : the hypotheses still in the distribution
 * The rule, for env e and watched agent a = agents[m]:
 *   1. initialise, with OC_BELIEF_INIT or when state_prev's flags carry OC_FLAG_DONE (the step
 *      auto-reset the env: oc_task_select's convention): open = every i < S whose kind is not
 *      OC_SUB_NONE, and bit S; live = open; every live belief = 1.0 / n_live (n_live = the number
 *      of live hypotheses), the others +0.0 (SubtaskAllocDistribution.__init__).  OC_BELF_REINIT;
 *      go to 7.
 *   2. reset priors, if events is given and events & open is non-zero (an open subtask was
 *      completed; agent.py:185-192 calls set_priors instead of bayes_update): open &= ~events;
 *      live = open; the beliefs uniform as in 1.  OC_BELF_RESET; go to 7.
 *   3. prune: a live i < S whose row {kind_i, num_agents 1, agent {a}, start_mask_i, goal_mask_i}
 *      is not doable on state_prev (exactly oc_subtask_bounds' doable byte) leaves live and its
 *      belief becomes +0.0.  OC_BELF_PRUNED.
 *   4. raise test, only if some i < S is still live: prob_nav_actions raises if the Level-0
 *      configuration for {a} raises (two other agents on one square, OC_POL_RAISES' first case) or
 *      if a's taken action is not in get_actions on that Level-0 view (the assert at :672); for
 *      one-agent hypotheses neither depends on i.  Then OC_BELF_RAISED, step 5 is skipped.
 *   5. multiply: for the live i ascending, belief_i = belief_i * L_i (one f64 multiply).  For
 *      i < S, L_i = p_taken of exactly the distribution oc_nav_policy defines for the row
 *      (state_prev[e], subtask i for agent a) with OC_POLICY_COUNT_STATE: m = min Q,
 *      w_k = exp(beta * (m - Q_k)), the sum ascending from +0.0, p = w / sum; the reference's
 *      softmax(beta * (Q_taken - Q_k))[taken] on a fresh planner configured on obs_tm1.  L_S is
 *      oc_nav_policy's None closed form: n = a's movable actions in the full state, L_S =
 *      p(no-op) if the taken action is the no-op, else p(each movable action); n = 0: 1 and 0.  (A
 *      live OC_SUB_NONE row inside the table takes L_S.)  OC_BELF_UPDATED.
 *   6. normalise (utils.py:186-193): total = +0.0 plus the live beliefs in ascending order; if
 *      total == 0 every live belief = 1.0 / n_live, else r = 1.0 / total and belief_i =
 *      belief_i * r (a multiply by the reciprocal, not a division).
 *   7. map = the lowest live i holding the maximum belief.
 * A second call without a step in between is not idempotent: it multiplies again.
 * ------------------------------------------------------------------------------------- */
#define OC_BELIEF_INIT 1         /* every env below B starts its episode: step 1 for all of them */
#define OC_BELF_UPDATED 0x01     /* step 5 ran */
#define OC_BELF_PRUNED  0x02     /* a hypothesis left the distribution in step 3 */
#define OC_BELF_REINIT  0x04     /* initialised in this call (step 1) */
#define OC_BELF_RESET   0x08     /* uniform priors over the open subtasks after a completion (step 2) */
#define OC_BELF_RAISED  0x10     /* the reference's likelihood raises: pruned and normalised only */
#define OC_BELIEF_PLANES(S) (((S) + 8) / 8)

/*   state_prev   : B states (oc_layout), the states the step left (oc_step's state_in)
 *   taken        : u8 [A][pitch], the executed actions of that step (oc_step's exec); codes > 4
 *                  act as the no-op
 *   events       : nullable, u8 [OC_PROGRESS_EVENT_PLANES(S)][pitch], oc_progress's events of that
 *                  same step over the same S rows
 *                  With OC_BELIEF_INIT state_prev, taken and events may be NULL (and are not read)
 *   subtasks     : host array of S = num_subtasks rows, 1 <= S <= 63; only kind, start_mask and
 *                  goal_mask are read (capi.progress_subtasks / policy_subtasks rows serve)
 *   agents       : host array of M = num_watched distinct agent indices, 1 <= M <= A; the watched
 *                  agents do not depend on each other
 *   beta, none_action_prob : as oc_nav_policy (none_action_prob in [0, 1])
 *   belief       : required, f64 [M][S + 1][pitch], 8-byte aligned, read and written in place
 *   bstate       : required, u8 [M][2 * HP][pitch], read and written in place: planes 0 .. HP-1
 *                  open, HP .. 2HP-1 live
 *   map          : nullable, u8 [M][pitch]
 *   info         : nullable, u8 [M][pitch], OC_BELF_* bits
 * Columns >= B of every buffer stay untouched; a belief plane is written only where step 1 or 2
 * ran or the hypothesis was live at entry.  Stream-ordered, no allocation, no synchronisation
 * (hipGraph-capturable, as oc_step).  Bad arguments and a host-only handle are OC_EINVAL; B = 0
 * is OK. */
int oc_belief_update(const oc_handle* h, const void* state_prev, const uint8_t* taken, const uint8_t* events,
                     const oc_subtask* subtasks, int32_t num_subtasks, const uint8_t* agents, int32_t num_watched,
                     double beta, double none_action_prob, int32_t flags, double* belief, uint8_t* bstate, uint8_t* map,
                     uint8_t* info, int64_t B, void* stream);

/* The same on the host (what oc_cpu_step is to oc_step): HOST buffers, works on OC_DEVICE_HOST
 * handles, the whole rule per (env, watched agent) as one scalar row function, threaded over env
 * ranges (nthreads 0 = the host's hardware threads; at least 1,024 rows each).  It never touches
 * the device; oc_belief_update never calls it.  The two agree on bstate, info and, up to the last
 * bits of exp and of a fused multiply-add, on belief. */
int oc_cpu_belief_update(const oc_handle* h, const void* state_prev, const uint8_t* taken, const uint8_t* events,
                         const oc_subtask* subtasks, int32_t num_subtasks, const uint8_t* agents, int32_t num_watched,
                         double beta, double none_action_prob, int32_t flags, double* belief, uint8_t* bstate,
                         uint8_t* map, uint8_t* info, int64_t B, int32_t nthreads);

/* ---------------------------------------------------------------------------------------
 * Per-env Bayesian belief over a pair's allocation (additive to ABI 12): Bayesian Delegation itself
 * (model `bd`) on the batch.  oc_belief_update reasons about "agent a alone follows subtask i"; this
 * call keeps the reference delegator's posterior over the whole allocation space of two agents,
 * "both on t" beside "a0 on i, a1 on j", updates it with the actions both agents executed, and maps
 * it to the three `alloc` planes of oc_team_select's format: the delegator then acts on its own
 * member of the most likely allocation.
 *   add_subtasks (the enumeration and its order)    delegation_planner/bayesian_delegator.py:697-886
 *   prune_subtask_allocs, subtask_alloc_is_doable   bayesian_delegator.py:200-256, :98-156
 *   bayes_update                                    bayesian_delegator.py:1026-1072
 *   prob_nav_actions (no_level_1)                   bayesian_delegator.py:461-689
 *   select_subtask                                  bayesian_delegator.py:1009-1017
 *   update_subtasks (set_priors after a completion) gym_cooking/utils/agent.py:176-203
 *   normalize, get_max                              delegation_planner/utils.py:186-215
 * Build-defined, and only these: uniform priors (the reference also offers spatial priors); the
 * likelihoods of a fresh planner configured on obs_tm1 with no_level_1 = True (oc_nav_policy's Q
 * values, not BRTDP-updated ones); ties of the maximum go to the first hypothesis in reference order
 * (get_max draws at random); and a None member whose self agent has no movable action (n = 0, where
 * the reference divides by zero) has likelihood 1 for the no-op and 0 otherwise.
 *
 * The pair is a0 = agents[0] < a1 = agents[1]; self_agent, the delegator, is a0 or a1.  With S =
 * num_subtasks, N = S + 1, EP = OC_PROGRESS_EVENT_PLANES(S) and HP = OC_BELIEF_PLANES(S), the
 * hypotheses form an N x N matrix, hypothesis (i, j) in plane i * N + j of `belief`:
 *   i != j     the split "a0 alone on subtask i, a1 alone on subtask j", index S meaning None
 *   i == j < S the joint "both on subtask i"
 *   (S, S)     no hypothesis: the plane is never read or written
 * Reference order is add_subtasks' order for two agents: the joints by ascending i, then the splits
 * in row-major (i, j).  OC_SUB_NONE rows inside the table are never hypotheses.
 * The state of an env is u8 [OC_TBELIEF_PLANES(S) = 2 EP + 2 HP][pitch], four bit sets in
 * oc_belief_update's numbering (bit b of plane c is index 8c + b):
 *   planes 0 .. EP-1          open : the subtasks nobody has completed this episode
 *   EP .. EP+HP-1             live0: a0's members still in the distribution, over 0 .. S
 *   EP+HP .. EP+2HP-1         live1: a1's
 *   EP+2HP .. 2EP+2HP-1       liveJ: the joint members
 * A split (i, j) is live iff live0 has i and live1 has j; a joint i iff liveJ has i.  The factored
 * form is exact: the reference deletes an allocation iff one of its members is not doable
 * (bayesian_delegator.py:1031-1038), and that is decided per member.  n_live counts the live
 * hypotheses.  The rule, for env e:
 *   1. initialise, with OC_TBELIEF_INIT or when state_prev's flags carry OC_FLAG_DONE: open = the
 *      rows whose kind is not OC_SUB_NONE; live0 = live1 = open plus bit S; liveJ = open; every live
 *      belief = 1.0 / n_live, every other plane of the matrix +0.0.  OC_TBELF_REINIT; go to 7.
 *   2. reset priors, if events is given and events & open is non-zero (agent.py:185-192): open &=
 *      ~events; the live sets from open and the beliefs uniform as in 1.  OC_TBELF_RESET; go to 7.
 *   3. prune: live0 loses i < S if the row {kind_i, 1 agent {a0}, masks_i} is not doable on
 *      state_prev (exactly oc_subtask_bounds' doable byte); live1 loses j likewise with {a1}; liveJ
 *      loses t likewise with {a0, a1}.  The belief of every hypothesis that left becomes +0.0, and
 *      OC_TBELF_PRUNED is set if one did.
 *   4. empty: if n_live is 0, OC_TBELF_EMPTY; go to 8 (the reference has nobody on anything).
 *   5. raise test.  The members form three families: a0's one-agent rows, a1's, and the pair's
 *      two-agent rows.  A family raises where oc_nav_likelihood would flag its rows OC_LIK_RAISES:
 *      its Level-0 configuration raises, the taken action (the pair's: the taken joint action) is not
 *      in get_actions on its Level-0 view, or a legal candidate's transition ends with the pair on
 *      one square.  None of these reads the subtask: interact, the legality tests and the removed
 *      agents depend on the family's agents only, for the two-agent rows as for the one-agent rows,
 *      so the test is made once per family.  If a family raises that has a subtask (not None) as
 *      a member of some live hypothesis: OC_TBELF_RAISED, and step 6 is skipped.
 *   6. multiply (one f64 add and one f64 multiply per live hypothesis; bayes_update's factor is the
 *      sum over the members of len(agents) * prob_nav_actions):
 *        split (i, j): belief = belief * (L0_i + L1_j);   joint t: belief = belief * (2.0 * LJ_t)
 *      Each L is oc_nav_likelihood's value for (state_prev, taken, the member's row, self_agent,
 *      beta, none_action_prob) with the goal count of state_prev's own Level-0 view
 *      (OC_POLICY_COUNT_STATE): over the legal candidates k, m = min Q_k, w_k = exp(beta * (m -
 *      Q_k)), the sum ascending from +0.0, L = w_taken / sum.  A one-agent row has the member's five
 *      actions as candidates.  For a joint row self is inside the pair, so the candidates are the
 *      five joint actions that keep the other member's taken action (:676-680), not 25.  For None,
 *      n is the *self* agent's movable actions in the full state (:621; the reference's quirk, and
 *      unlike oc_belief_update) while the tested action is the member's: oc_nav_policy's closed
 *      form, p(no-op) if the member's taken action is the no-op, else p(each movable action).
 *      OC_TBELF_UPDATED.
 *   7. normalise (utils.py:186-193): total = +0.0 plus the live beliefs in reference order; if total
 *      is 0 every live belief = 1.0 / n_live, else each is multiplied by 1.0 / total.  That order
 *      is the host call's.  The device call adds each lane's hypotheses (row-major, columns j = lane
 *      mod 8) and then the 8 lanes' sums pairwise, so its total, and every belief with it, can
 *      differ from the host's in the last bits: the two are tested to agree to 1e-12.
 *   8. map = the first hypothesis in reference order holding the maximum, as oc_team_select's
 *      (cur0, cur1, curJ): a joint t is (OC_TEAM_OUT, OC_TEAM_OUT, t), a split (i, j) is
 *      (i, j, OC_TEAM_OUT), nothing live is the idle split (S, S, OC_TEAM_OUT).  The three planes are
 *      directly the `alloc` planes of three oc_nav_policy launches.  OC_TBELF_JOINT iff it is joint.
 * A second call without a step in between is not idempotent: it multiplies again.
 * Memory: the belief matrix is (S + 1)^2 * 8 bytes per env, 839 MB at S = 9 and 2^20 envs.
 * ------------------------------------------------------------------------------------- */
#define OC_TBELIEF_INIT 1         /* every env below B starts its episode: step 1 for all of them */
#define OC_TBELF_UPDATED 0x01     /* step 6 ran */
#define OC_TBELF_PRUNED  0x02     /* a hypothesis left the distribution in step 3 */
#define OC_TBELF_REINIT  0x04     /* initialised in this call (step 1) */
#define OC_TBELF_RESET   0x08     /* uniform priors over the open subtasks after a completion (step 2) */
#define OC_TBELF_RAISED  0x10     /* the reference's likelihood raises: pruned and normalised only */
#define OC_TBELF_EMPTY   0x20     /* step 3 left no hypothesis (step 4) */
#define OC_TBELF_JOINT   0x40     /* the map is a joint allocation */
#define OC_TBELIEF_PLANES(S) (2 * OC_PROGRESS_EVENT_PLANES(S) + 2 * OC_BELIEF_PLANES(S))

/*   state_prev, taken, events : as oc_belief_update (with OC_TBELIEF_INIT all three may be NULL)
 *   subtasks     : host array of S = num_subtasks rows, 1 <= S <= OC_TEAM_MAX_SUBTASKS; only kind,
 *                  start_mask and goal_mask are read
 *   agents       : host array of 2 agent indices, a0 < a1 < A (so A >= 2)
 *   self_agent   : the delegator, a0 or a1
 *   beta, none_action_prob : as oc_nav_policy (none_action_prob in [0, 1])
 *   belief       : required, f64 [N * N][pitch], 8-byte aligned, read and written in place
 *   tbstate      : required, u8 [OC_TBELIEF_PLANES(S)][pitch], read and written in place
 *   lik          : nullable, f64 [3 S + 2][pitch], 8-byte aligned: the step's L0 (planes 0 .. S),
 *                  L1 (N .. N + S) and LJ (2 N .. 2 N + S - 1), written where step 6 ran: +0.0 for a
 *                  member outside its live set or whose family raises
 *   map          : nullable, u8 [3][pitch]: cur0, cur1, curJ
 *   info         : nullable, u8 [pitch], OC_TBELF_* bits
 * Columns >= B of every buffer stay untouched; a belief plane is written only where step 1 or 2 ran
 * or the hypothesis was live at entry.  Stream-ordered, no allocation, no synchronisation
 * (hipGraph-capturable, as oc_step).  Bad arguments, A = 1 and a host-only handle are OC_EINVAL;
 * B = 0 is OK. */
int oc_team_belief_update(const oc_handle* h, const void* state_prev, const uint8_t* taken, const uint8_t* events,
                          const oc_subtask* subtasks, int32_t num_subtasks, const uint8_t* agents, int32_t self_agent,
                          double beta, double none_action_prob, int32_t flags, double* belief, uint8_t* tbstate,
                          double* lik, uint8_t* map, uint8_t* info, int64_t B, void* stream);

/* The same on the host (what oc_cpu_step is to oc_step): HOST buffers, works on OC_DEVICE_HOST
 * handles, the whole rule per env as one scalar row function, threaded over env ranges (nthreads
 * 0 = the host's hardware threads; at least 1,024 rows each).  It never touches the device;
 * oc_team_belief_update never calls it.  The two agree on tbstate and info byte for byte and, up to
 * the last bits of exp, of a fused multiply-add and of the order of step 7's sum (the device adds
 * per lane, then across lanes), on belief and lik; map, and with it OC_TBELF_JOINT, is each call's
 * first maximum of its own beliefs (L0_i + L1_j and 2 LJ_t can be one ulp apart). */
int oc_cpu_team_belief_update(const oc_handle* h, const void* state_prev, const uint8_t* taken, const uint8_t* events,
                              const oc_subtask* subtasks, int32_t num_subtasks, const uint8_t* agents,
                              int32_t self_agent, double beta, double none_action_prob, int32_t flags, double* belief,
                              uint8_t* tbstate, double* lik, uint8_t* map, uint8_t* info, int64_t B, int32_t nthreads);

#ifdef __cplusplus
}
#endif

#endif /* OC_ENGINE_H_ */
