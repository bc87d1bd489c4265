/*
 * hk.h — C ABI of libhk.so: the MI355X-native batched kart-racing step + feedback LQ Nash-game solve.
 *
 * Drop-in boundary for ONE hot path of ribsthakkar/HierarchicalKarting (Unity C#).  The reference has no FFI for
 * this path (everything is in-process managed calls), so each entry point below names the managed surface it
 * replaces (reference file:line, paths relative to Assets/Karting/Scripts/).  A C# host binds these with
 * [DllImport("hk")]; all types are blittable (int32 / uint32 / float / double / pointers).
 *
 * Conventions: return 0 on success, negative hk_status on error (never throws across the ABI);
 * host buffers are caller-owned, device buffers library-owned; one handle = one GPU context, NOT thread-safe
 * (Unity drives it from FixedUpdate on the main thread, like the reference); row-major arrays.
 * There is NO CPU fallback: without a HIP device hk_create / hk_lq_solve_batch fail with HK_ERR_NO_DEVICE.
 */
#ifndef HK_H
#define HK_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HK_ABI_VERSION 6
#define HK_MAX_AGENTS 8      /* the largest reference scene has 4; 5..8 agents per env is the synthetic extension of BASELINE configs[4] (start grid continued row by row) */
#define HK_MAX_SECTIONS 64   /* Oval 24, Complex 41 */
#define HK_NUM_SENSORS 9     /* MLAgent_Sensors.prefab */

typedef enum hk_status {
    HK_OK = 0,
    HK_ERR_INVALID = -1,      /* bad argument / config */
    HK_ERR_NO_DEVICE = -2,    /* no HIP device: the product path has no CPU fallback */
    HK_ERR_HIP = -3,          /* HIP runtime error (see hk_last_error) */
    HK_ERR_UNSUPPORTED = -4,  /* valid in the reference, not built yet (num_agents > 4, LQ games of > 8 players) */
    HK_ERR_SINGULAR = -5      /* LQ: zero pivot in the m x m solve */
} hk_status;

/* HierarchicalKartAgent.cs:21-33.  HK_LOW_E2E: the slot is an EndToEndKartAgent (AI/EndToEndKartAgent.cs) instead — actions from the
 * ML-Agents brain only (no LQ game, no planFixed), its own observation layout and reward path; its high_mode is then HK_HIGH_MCTS
 * (runQuasiMCTS on: planWithMCTS every 100 ticks with the agent's own gameParams, no plan at reset; the plan feeds the lane / velocity
 * difference metrics only) or HK_HIGH_NONE (runQuasiMCTS off).  HK_HIGH_NONE is valid only with HK_LOW_E2E. */
enum { HK_LOW_RL = 0, HK_LOW_MPC = 1, HK_LOW_LQR = 2, HK_LOW_E2E = 3 };
enum { HK_HIGH_MCTS = 0, HK_HIGH_FIXED = 1, HK_HIGH_NONE = 2 };
/* RacingEnvController.cs:24-29 */
enum { HK_MODE_RACE = 0, HK_MODE_TRAINING = 1, HK_MODE_EXPERIMENT = 2 };

/* agent flag bits (hk_agent_state.flags) */
enum {
    HK_F_ACCEL = 1u << 0,             /* KartAgent.m_Acceleration      KA:104 */
    HK_F_BRAKE = 1u << 1,             /* KartAgent.m_Brake             KA:105 */
    HK_F_ACTIVE = 1u << 2,            /* KartAgent.is_active           KA:123 */
    HK_F_FORWARD_COLLISION = 1u << 3, /* KartAgent.forwardCollision    KA:125 */
    HK_F_HAS_COLLISION = 1u << 4,     /* ArcadeKart.m_HasCollision     AK:202 */
    HK_F_CAN_MOVE = 1u << 5,          /* ArcadeKart.m_CanMove          AK:195 */
    HK_F_ENABLED = 1u << 6            /* GameObject.activeSelf (Deactivate(disable) KA:405-416) */
};

/* ArcadeKart.Stats (KartSystems/ArcadeKart.cs:20-69); values used: SURVEY App. A */
typedef struct hk_kart_stats {
    float TopSpeed, Acceleration, ReverseSpeed, ReverseAcceleration, AccelerationCurve, Braking, CoastingDrag, Grip;
    float MaxSteer, MinSteer, TireWearFactor, MinGs, MaxGs, AddedGravity;
    float TireWearRate;      /* AK:191 */
    float AngularDrag;       /* Rigidbody.angularDrag 0.05 (BaseKartClassic.prefab:173) */
} hk_kart_stats;

/* one DiscretePositionTracker (DiscretePositionTracker.cs:20-44) with its Waypoint prefab geometry */
typedef struct hk_section {
    float trig_x, trig_z;        /* Trigger box centre (box 10 x 1 x 1, local z +0.407 from the waypoint) */
    float yaw_deg;               /* Unity Y rotation of the waypoint (0 = +z, 90 = +x) */
    float marker_y;              /* world y of Trigger / lane markers (0.75): the constant dy of quirk Q13 */
    float lane_x[4], lane_z[4];  /* Lane1..Lane4 markers */
    float track_inside_radius, track_length, track_width, turn_degrees;
    int32_t left_turn, optimal_lane;
} hk_section;

typedef struct hk_wall_seg { float x0, z0, x1, z1; } hk_wall_seg; /* road-side wall face, world metres */

/* RacingEnvController reward fields (REC:65-108, defaults as in the source) */
typedef struct hk_reward_params {
    float WallHitPenalty, OpponentHitPenalty, HitByOpponentPenalty, PassCheckpointLaneReward, PassCheckpointVelocityReward;
    float PassCheckpointBase, PassCheckpointTimeMultiplier, TeamPassCheckpointBase, TeamPassCheckpointTimeMultiplier;
    float BeingBehindOpponentCheckpointPenalty, BeingBehindTeammateCheckpointPenalty, TeamScoreRewardMultiplier;
    float ReversePenalty, SwervingPenalty, ReachGoalCheckpointRewardMultplier, ReachGoalCheckpointRewardBase;
    float TowardsCheckpointReward, SpeedReward, SlowMovingPenalty, AccelerationReward, NotAtGoalPenalty;
} hk_reward_params;

/* Engine restatement: what Unity / PhysX does between two FixedUpdates and the C# never spells out.  Every
 * constant is read from the reference's prefabs / assets; `side_slope0` is the one fitted number.
 *   rigid body   Rigidbody mass 250, free rotation (m_Constraints 0; BaseKartClassic.prefab:164-178); centre of mass = the
 *                WheelColliders transform, kart-local (0, 0.12, 0) (AK:254, BaseKartClassic.prefab:203); inertia about y = that of the
 *                capsule collider (r 0.45, h 2, axis z) at mass 250 = 74.7 kg m^2 (PhysX computes it from the shapes)
 *   contacts     kart capsule: PhysicsMaterials/NoFriction (friction 0, bounciness 0); track MeshColliders: CarWheels (friction 0,
 *                combine Minimum) -> frictionless, inelastic contacts; an off-centre contact impulse turns the body
 *   wheels       four WheelColliders (BaseKartClassic.prefab:35-63,...): axles at kart-local z +0.586 / -0.681, sidewaysFriction
 *                {extremum (0.2, 1), asymptote (0.5, 0.75), stiffness 1}; the front pair is steered by KartAnimation.FixedUpdate
 *                (KartAnimation.cs:54-63): steerAngle = MoveTowards(smoothed, TurnInput, 10 dt) * maxSteeringAngle 30 */
typedef struct hk_engine_params {
    float mass, inertia_y, gravity;
    float axle_zf, axle_zr;          /* front / rear axle, metres ahead of the centre of mass */
    float max_steer_deg;             /* KartAnimation.maxSteeringAngle */
    float steer_damping;             /* KartAnimation.steeringAnimationDamping (1 / s) */
    float side_ext_slip, side_ext_value, side_asy_slip, side_asy_value, side_stiffness;   /* WheelCollider.sidewaysFriction */
    float side_slope0;               /* FITTED: slope of the friction curve at zero slip, in units of ext_value / ext_slip (0 .. 3) */
    float slip_min_speed;            /* m/s added to |longitudinal speed| in the slip ratio (PhysX vehicle tire model: 1) */
    /* rolling: no script drives or brakes the wheels (motorTorque = brakeTorque = 0), so their spin follows the ground through the
     * forwardFriction curve and is damped by wheelDampingRate; the force that keeps them turning is a drag on the body, and every change
     * of the kart's speed has to spin 4 x 20 kg of wheel up or down */
    float wheel_mass;                /* WheelCollider.mass 20 (moment of inertia m r^2 / 2) */
    float wheel_radius_f, wheel_radius_r;   /* 0.1372984 / 0.1630791 */
    float wheel_damping;             /* WheelCollider.wheelDampingRate 0.56 (kg m^2 / s) */
    float fwd_ext_slip, fwd_ext_value, fwd_asy_slip, fwd_asy_value, fwd_stiffness;        /* WheelCollider.forwardFriction */
    float long_slip_min_speed;       /* m/s added to |longitudinal speed| in the longitudinal slip ratio (PhysX minLongSlipDenominator: 4) */
    int32_t wheel_friction;          /* 0: no tire forces (the model of ABI <= 4) */
    int32_t contact_yaw;             /* 0: contacts change the linear velocity only (the model of ABI <= 4) */
    int32_t wheel_rolling;           /* 0: no longitudinal tire forces */
} hk_engine_params;

typedef struct hk_config {
    int32_t abi_version;         /* HK_ABI_VERSION */
    int32_t num_envs;            /* E: independent RacingEnvControllers on this device */
    int32_t num_agents;          /* A: RacingEnvController.Agents.Length (REC:49) */
    int32_t device_id;
    /* wiring: KartAgent.teamAgents / otherAgents (KA:63-65), RacingEnvController.Teams (REC:46) */
    int32_t team_of[HK_MAX_AGENTS];
    int32_t n_team[HK_MAX_AGENTS];
    int32_t team_agents[HK_MAX_AGENTS][HK_MAX_AGENTS];
    int32_t n_other[HK_MAX_AGENTS];
    int32_t other_agents[HK_MAX_AGENTS][HK_MAX_AGENTS];
    int32_t high_mode[HK_MAX_AGENTS];          /* HK_HIGH_*  (HKA:64) */
    int32_t low_mode[HK_MAX_AGENTS];           /* HK_LOW_*   (HKA:62) */
    int32_t tree_search_depth[HK_MAX_AGENTS];  /* gameParams.treeSearchDepth (HKA:48) */
    int32_t velocity_bucket_size[HK_MAX_AGENTS];
    hk_kart_stats stats;                       /* identical on every kart of the Compete scenes */
    /* rules (REC:110-130) */
    int32_t laps, max_episode_steps, max_lane_changes, section_horizon, disable_on_end, env_mode;
    int32_t start_hold_ticks;    /* WaitForSeconds(1.5f) at dt 0.02 = 75 ticks (REC:721-724) */
    int32_t auto_reset;          /* REC.FixedUpdate resets when every agent is inactive (REC:241-270) */
    float dt;                    /* Time.fixedDeltaTime 0.02 */
    float kart_y;                /* spawn height 0.28 (REC:715) */
    /* sensors (MLAgent_Sensors.prefab, KA:20-26): yaw in degrees, positive = to the right */
    float sensor_yaw_deg[HK_NUM_SENSORS];
    float ray_distance[HK_NUM_SENSORS];
    float wall_hit_validation[HK_NUM_SENSORS];
    float agent_hit_validation[HK_NUM_SENSORS];
    /* synthetic de-synchronisation of the start grid (NOT in the reference): Philox-4x32 keyed by
     * jitter_seed + env_id;  dx,dz ~ U(-jitter_pos, jitter_pos), dyaw ~ U(-jitter_yaw, jitter_yaw) rad. 0 = off. */
    uint32_t jitter_seed;
    float jitter_pos, jitter_yaw;
    int32_t env_id_base;         /* global id of local env 0 (multi-GPU sharding: contiguous ranges per rank) */
    /* track */
    int32_t num_sections;
    int32_t num_walls;
    const hk_section* sections;
    const hk_wall_seg* walls;
    /* MCTS high-level planner (HighMode == HK_HIGH_MCTS; KartMCTS.cs, KartDiscreteGame.cs, HKA:172-284,330-402).
     * gameParams (HKA:38-52), scene values {timePrecision 100, sectionWindow 2, treeSearchDepth 8, velocityBucketSize 2}.
     * The reference searches on a background thread under a WALL-CLOCK budget (T = 1.5 s at reset, 0.9 s every 100
     * ticks) with System.Random / MathNet draws; here the budget is an iteration count, the plan becomes visible a fixed
     * number of ticks after it was requested, and the draws are Philox-4x32 keyed by mcts_seed ("parity unpinned").  Root reuse
     * (HKA:265-283) and the sectionTimes back-fill of ResetGame (REC:679-702) are restated; see hk_mcts_state. */
    int32_t time_precision[HK_MAX_AGENTS];
    int32_t section_window[HK_MAX_AGENTS];
    int32_t mcts_iterations;          /* search iterations of a 100-tick replan (stands for T = 0.9 s) */
    int32_t mcts_initial_iterations;  /* of the plan made at reset (T = 1.5 s) */
    int32_t mcts_latency_ticks;       /* ticks until a replan's result is used (0.9 s = 45 ticks) */
    int32_t mcts_initial_latency_ticks;/* same for the plan made at reset (1.5 s = 75 ticks = the start hold) */
    uint32_t mcts_seed;
    /* reward shaping: 0 = off (hk_agent_state reward fields stay 0) */
    int32_t rewards;
    int32_t training_agent[HK_MAX_AGENTS];   /* KartAgent.Mode == AgentMode.Training (KA:34-38): only these enter AddGoalTimingRewards (REC:217) */
    hk_reward_params rw;
    /* env_mode == HK_MODE_TRAINING: ResetGame scatters the karts at random (REC:520-668); training_agent[i]: the agent plans
     * with planRandomly (HKA:109-143) instead of planFixed / MCTS.  UnityEngine.Random / System.Random draws become
     * Philox-4x32 keyed by train_seed, the global env id and the episode ("parity unpinned"). */
    uint32_t train_seed;
    int32_t debug_taps;          /* bit 0: record the LQ debug taps read by hk_get_lq_debug (costs a few %).  The environment variable
                                  * HK_LQ_DEBUG=<bits>, read once by hk_create, ORs into this field (tests switch the taps on without
                                  * rebuilding their configs) */
    hk_engine_params engine;     /* ABI 5 */
} hk_config;

#define HK_MCTS_MAX_DEPTH 8      /* gameParams.treeSearchDepth <= 8 */
#define HK_MCTS_MAX_ACTIONS 36   /* velocity buckets x 4 lanes (KartDiscreteGame.cs:329-338: for (i = 6; i < 15; i += velocityBucketSize)): 5 x 4 at
                                  * velocityBucketSize 2 (the MCTS-LQR agents of the Compete scenes), 9 x 4 at 1 (their MCTS-RL / Fixed-RL agents) */
#define HK_MCTS_SECTIME_RING 8   /* sectionTimes entries kept per kart (sectionWindow <= 4) */
#define HK_MCTS_MAX_ROOT_PHASES 3 /* searches one tree can receive (the reference: CyclesRootProcessed < 3); see hk_mcts_state.root_phases */

/* Planner state of one agent (kept beside hk_agent_state; HighMode MCTS agents only).  `best` is what the reference
 * holds in bestStates (HKA:70,252): for each future section the game reached by every player, each player's lane and
 * max_velocity; `pend` is a finished search that becomes `best` at episode step ready_step. */
typedef struct hk_mcts_plan {
    int32_t n_states;                                  /* 0..HK_MCTS_MAX_DEPTH */
    int32_t n_players;
    int32_t section[HK_MCTS_MAX_DEPTH];                /* lastCompletedSection of the state */
    uint8_t player_agent[HK_MAX_AGENTS];               /* Agents[] index of each player */
    uint8_t lane[HK_MCTS_MAX_DEPTH][HK_MAX_AGENTS];
    uint8_t vel[HK_MCTS_MAX_DEPTH][HK_MAX_AGENTS];     /* max_velocity */
} hk_mcts_plan;

typedef struct hk_mcts_state {
    int32_t sec_time[HK_MCTS_SECTIME_RING];            /* KartAgent.sectionTimes (KA:124), ring over section & 7: the planner reads the
                                                        * entries of karts at most 2 * sectionWindow - 2 <= 6 sections apart (HKA:221-224) */
    int32_t ready_step;                                /* episode step at which `pend` replaces `best`; -1: nothing pending */
    int32_t searches;                                  /* searches started since hk_create (debug / RNG stream id) */
    /* root reuse (HKA:66-67,175,265-283,660-669): a replan re-searches the tree of the previous plan (up to three searches per
     * tree) unless the kart entered a section, or drove backwards through one, after that plan was finished */
    int32_t root_live;                                 /* currentRoot != null */
    int32_t root_cycles;                               /* CyclesRootProcessed */
    int32_t pend_kind;                                 /* the search in flight: 0 none, 1 a new tree (HKA:175), 2 the existing root again (HKA:265) */
    int32_t root_phases;                               /* searches the current tree has received (set at the request; <= HK_MCTS_MAX_ROOT_PHASES) */
    hk_mcts_plan best, pend;
    /* opponentUpcomingLanes / opponentUpcomingVelocities (HKA:77-78): this agent's belief about every other agent's
     * plan, keyed by section % L; 0 = no entry.  (HK_LOW_E2E rows: filled the same way but never read — the E2E agent keeps no beliefs) */
    uint8_t belief_lane[HK_MAX_AGENTS][HK_MAX_SECTIONS];
    uint8_t belief_vel[HK_MAX_AGENTS][HK_MAX_SECTIONS];
} hk_mcts_state;


/* Per-agent persistent state: the fields of KartAgent (KA:102-128), ArcadeKart (AK:190-205) and the Rigidbody that
 * survive a tick.  hk_get/set_agent_state copy every field, which gives snapshot/restore for free.  (On the device the fields that
 * change every tick live in a wave-tiled structure-of-arrays layout; this record is the host-facing view.) */
typedef struct hk_agent_state {
    float px, pz;                 /* transform.position (x, z); y is kart_y */
    float yaw;                    /* Unity Y rotation, radians, kept in [0, 2pi) */
    float vx, vz;                 /* Rigidbody.velocity */
    float wy;                     /* Rigidbody.angularVelocity.y (rad/s) */
    float acc_ang_v;              /* ArcadeKart.m_AccumulatedAngularV (AK:190) */
    float steering;               /* KartAgent.m_Steering (KA:106) */
    float avg_lane_diff;          /* KA:116 */
    float avg_vel_diff;           /* KA:115 */
    float cum_reward;             /* Agent.GetCumulativeReward(): sum of AddReward since the episode began (0 unless cfg.rewards) */
    float contact_nx, contact_nz; /* m_LastCollisionNormal (AK:201), x/z */
    int32_t section_index;        /* m_SectionIndex KA:107 */
    int32_t lane;                 /* m_Lane KA:108 */
    int32_t lane_changes;         /* KA:109 */
    int32_t illegal_lane_changes; /* KA:110 */
    int32_t forward_collisions;   /* KA:126 */
    int32_t last_collision_time;  /* KA:127 */
    int32_t time_steps;           /* m_timeSteps KA:112 */
    int32_t init_checkpoint_index;/* KA:49 */
    uint32_t flags;               /* HK_F_* */
    uint32_t trig_lo, trig_hi;    /* which Trigger boxes the kart overlapped after the last tick (OnTriggerEnter edge) */
    float final_steer;            /* ArcadeKart.m_FinalStats.Steer as of the last UpdateStats (AK:300) */
    /* TelemetryViewer per-agent arrays (TelemetryViewer.cs:12-16), advanced once per tick after the engine step */
    int32_t tele_completed_laps;  /* lastCompletedLaps */
    int32_t tele_lap_end_step;    /* lastEpisodeSteps */
    float tele_last_lap;          /* lastLapTimes (s) */
    float tele_best_lap;          /* bestLapTimes (s) */
    float tele_total_time;        /* lastOverallTimes (s) */
    uint8_t plan_lane[HK_MAX_SECTIONS]; /* m_UpcomingLanes keyed by section % L (KA:117); 0 = no entry */
    float plan_vel[HK_MAX_SECTIONS];    /* m_UpcomingVelocities (KA:118) */
    /* ML-Agents per-decision accumulators: what Agent.AddReward / AddGroupReward collected since hk_get_rewards last
     * read them (Agent.SendInfo resets m_Reward / m_GroupReward the same way) */
    float step_reward;
    float group_reward;
    float steer_smoothed;         /* KartAnimation.m_SmoothedSteeringInput (KartAnimation.cs:43,56): the front WheelColliders' steerAngle / 30 deg (ABI 5) */
    float wheel_uf, wheel_ur;     /* rim speed (angular velocity x radius, m/s) of the front / rear WheelCollider pair (ABI 5) */
} hk_agent_state;

typedef struct hk_env_state {
    int32_t episode_steps;     /* REC:125 */
    uint32_t inactive_mask;    /* REC.inactiveAgents (REC:118) as a bit set over Agents[] */
    int32_t experiment_num;    /* REC:63 */
    int32_t episodes_done;     /* finished episodes since hk_create */
    uint32_t status;           /* bit0 NaN/Inf seen in a kart state, bit1 timeout ended last episode */
    int32_t initial_started;   /* REC.initialStarted (REC:132): the very first all-inactive tick resets without logging */
    int32_t reserved[2];       /* library-internal progress words of hk_step: [0] ticks left, [1] bits 0..3 phase inside a tick (both 0 between calls), bit 4 a scheduling hint */
} hk_env_state;

/* TelemetryViewer / experiment-log quantities of the last finished episode (TelemetryViewer.cs:49-108) */
typedef struct hk_episode_result {
    int32_t time_steps;            /* m_timeSteps at finish; 0 = did not finish (REC:470,476) */
    int32_t section_index;         /* laps = section_index / L */
    int32_t illegal_lane_changes;
    int32_t forward_collisions;
    float avg_lane_diff;
    float avg_vel_diff;
    float reward;                  /* Agent.GetCumulativeReward() at the end of the episode */
    int32_t episode;               /* index of the episode these numbers belong to (-1: none finished yet) */
    float last_lap, best_lap, total_time;   /* TelemetryViewer.cs:58-79 (seconds) */
    int32_t laps_completed;        /* lastCompletedLaps */
    int32_t lap_end_step;          /* lastEpisodeSteps (enters the reference's winner rule, TelemetryViewer.cs:80) */
    float speed;                   /* Rigidbody.velocity.magnitude when the block was written */
    int32_t active;                /* is_active when the block was written */
    float group_reward;            /* m_GroupReward when the episode ended, AddGoalTimingRewards (REC:174-237) included: the record is
                                      rewritten by ResetGame in the same tick, so this is where a trainer finds the terminal group reward */
} hk_episode_result;

/* debug tap: the LQ game one ego assembled on its last solve tick (HKA:699-1201), ego-local player order */
typedef struct hk_lq_debug {
    int32_t n_players;
    int32_t player_agent[HK_MAX_AGENTS]; /* agent index of each player, order [this, team..., other...] filtered (HKA:702-725) */
    int32_t branch[HK_MAX_AGENTS];       /* heading-heuristic branch id B1..B7 per player */
    double initial[HK_MAX_AGENTS][4];
    double target[HK_MAX_AGENTS][4];
    double target_w[HK_MAX_AGENTS][4];
    double control_w[HK_MAX_AGENTS];
    double u0[2];
} hk_lq_debug;

typedef struct hk_context* hk_handle;

/* replaces: scene instantiation of RacingEnvController + KartAgents (REC.Start :148-168, HKA.Awake :413-426) */
int hk_create(const hk_config* cfg, hk_handle* out);
void hk_destroy(hk_handle h);
const char* hk_last_error(hk_handle h);

/* RacingEnvController.ResetGame (REC:499-719) for the listed envs (env_ids == NULL: all), Experiment/Race grid:
 * ordering = allOrderings[experiment_num % A!] (REC:528-530).  experiment_num < 0: per-env (env_id_base + env) % A! */
int hk_reset(hk_handle h, const int32_t* env_ids, int n, int experiment_num);

/* KartAgent.OnActionReceived / InterpretDiscreteActions (KA:440-478, HKA:1371-1379): only read by LowMode == RL agents.
 * steer[E][A] continuous action 0, branch[E][A] discrete action 0 in {0 brake, 1 coast, 2 accelerate} */
int hk_set_actions(hk_handle h, const float* steer, const int32_t* branch);

/* n_ticks Unity FixedUpdate ticks: REC.FixedUpdate -> [HKA.FixedUpdate incl. SolveLQR] ->
 * ArcadeKart.FixedUpdate -> engine step (integrate, contacts, triggers). Asynchronous on the handle's stream.
 * Completion.  hk_step returns when the work is ISSUED.  Calls of fewer than 64 ticks, and every call of a handle with a planner or
 * an attached actor, issue a fixed number of kernel rounds (the solve ticks the call can hold + 1) and need no host sync.  Calls of
 * >= 64 ticks of plain handles issue the rounds a field without queued games needs and leave the rest to the NEXT entry point that
 * touches the state (any hk_get_* / hk_set_* / hk_reset / hk_step / hk_prof_read / hk_gather_results, or hk_synchronize): it waits
 * for a two-word report of the device and issues what the laggard envs still need ("lazy completion").  hk_synchronize is the
 * completion point: a host that overlaps its own work with hk_step, or times it, calls hk_synchronize where it needs the ticks done.
 * A lazily completed call (>= 64 ticks) paces itself: the host stays about 8 rounds (32 ticks) of launches ahead of the GPU at most (a marker event
 * every 4 rounds, a wait for the marker two back) so that it can look at the games meter and change where multi-player games are solved while the call runs —
 * such a call returns when its LAST ~8 rounds are issued, not at once.  Shorter calls return as soon as they are issued.
 * Round 5: a fixed-round call of a plain handle whose envs are all believed to stand on the same episode step (a reset of every env, then only hk_step
 * calls) issues exactly the launches such a field needs — a one-tick call off a solve tick is one launch — and the completion guard verifies the
 * belief: the next entry point other than hk_step looks at it and, if an env fell behind (it finished its race, a time-out), finishes that env the
 * lazy way before anything is read.  Successive hk_step calls do not look; hk_synchronize does.
 * Error surface: hk_step only reports launch errors.  A completion guard (env_check_kernel, or the last tick launch of a fixed-round call) runs after the rounds of a call; if an
 * env still had ticks to run (an internal scheduling error) the next hk_get_agent_state / hk_get_env_state fails ONCE with
 * HK_ERR_HIP "an env did not complete its ticks" instead of returning stale state; the flag is sticky until that report (or
 * hk_reset), and the unfinished envs keep their leftover ticks, which the next hk_step runs first.  A zero pivot in an LQ solve is
 * sticky in the same way (status bit 0) but does not fail the getters: the reference throws nothing there either (MathNet returns
 * inf / NaN), and hk_env_state.status bit 0 flags the karts whose state went non-finite.
 * Scheduling switches, read from the environment ONCE in hk_create (none changes a result bit; hk_schedule_info() reports what a call ran):
 * HK_FISSION (0: every handle on the fused tick kernel instead of the tick kernel without phase B1 + env_b1_kernel per solve cadence), HK_SPLIT (0: one stream
 * always; unset: every call of a plain handle of >= 8 192 envs as two halves on two streams, joined into hk_stream by the next entry point that needs the whole
 * state), HK_INWAVE (0: multi-player games through the queues and a solver launch, 1: solved by the
 * B1 waves that assembled them in every round; unset: in-wave once the field has spread), HK_LQN (pair: the pair / matrix-core solver launch also for a spread
 * field), HK_FIXED_ROUNDS, HK_NO_OPTIMISTIC (fixed-round calls issue the worst-case round count instead of the verified plan of a field in lock-step),
 * HK_OPTIMISTIC_SKEW (tests), HK_MCTS_NO_PAUSE, HK_MCTS_NO_OVERLAP / HK_MCTS_SIDE_WAVES (a replan's searches on the handle's stream after the stretch / search
 * workgroup size beside the ticks); read at table / buffer set-up: HK_MCTS_PERSIST_GB, HK_NO_HOLD_DEDUPE, HK_LQ_DEBUG,
 * HK_TAB_GLOBAL (track tables read from global memory, as for tracks that exceed the LDS budget).  Round 6 retired the switches whose A/B was settled
 * (profiles/README.md keeps their numbers).
 * Planner handles (any HighMode MCTS agent): a call of more than 38 ticks without attached actors synchronises with the host
 * between stretches of ~100 ticks — envs wait at the tick boundary after a search request so that the searches of a stretch run
 * as ONE batch (results do not depend on it; environment variable HK_MCTS_NO_PAUSE=1 restores the fully asynchronous schedule).
 * Where the planner's trees live is decided at hk_create: one arena slice per agent if that fits HK_MCTS_PERSIST_GB (environment,
 * default 64), else one per resident search lane with re-searched roots rebuilt by replay; plans are bit-identical either way. */
int hk_step(hk_handle h, int n_ticks);

/* HierarchicalKartAgent.CollectObservations (HKA:485-604): obs[E][A][hk_obs_dim], order exactly as the reference adds them.
 * HK_LOW_E2E rows hold EndToEndKartAgent.CollectObservations (E2E:279-376) in the same hk_obs_dim: own block speed, accel, lane,
 * laneChanges / max, is_active, isStraight, tireWear, section / goal; the section horizon is always the Trigger (then 1, isStraight). */
int hk_obs_dim(hk_handle h);
int hk_get_observations(hk_handle h, float* obs);

int hk_get_agent_state(hk_handle h, hk_agent_state* out /*[E][A]*/);
int hk_set_agent_state(hk_handle h, const hk_agent_state* in /*[E][A]*/);   /* (MCTS agents: bestStates are copied into the new records on the next tick) */
int hk_get_env_state(hk_handle h, hk_env_state* out /*[E]*/);
int hk_set_env_state(hk_handle h, const hk_env_state* in /*[E]*/);            /* (reserved[0] is stored as 0 and reserved[1] keeps its hint bit only: the progress words are the library's) */
int hk_get_episode_results(hk_handle h, hk_episode_result* out /*[E][A]*/);
/* Agent.SendInfo: reward[E][A] = m_Reward, group_reward[E][A] = m_GroupReward collected since the last call; both reset to 0 */
int hk_get_rewards(hk_handle h, float* reward, float* group_reward);
int hk_get_lq_debug(hk_handle h, int env, int ego, hk_lq_debug* out);
/* planner state of every agent, [E][A] (zeros for agents that are not HighMode MCTS).  Searches are batched over hk_step calls
 * (at most 32 armed ticks, well inside the 41+ ticks a plan has until it is due): this call runs whatever is still queued first,
 * so `pend` always holds the result of the last request. */
int hk_get_mcts_state(hk_handle h, hk_mcts_state* out /*[E][A]*/);

/* KartLQR.solveFeedbackLQR (AI/LQR/KartLQR.cs:17) batched, 1:1 incl. quirks Q1 (block-transposed LHS) and Q2.
 * A[b][N][4][4], B[b][N][4][2], Q[b][N][n][n], q[b][N][n], R[b][N][2][2], x0[b][n], n = 4N; u0_out[b][2].
 * Host pointers; h may be NULL (a temporary context on device 0 is used). N <= 8
 * (the env path uses N <= 4 = agents per env; 5..8 run the same generic core, untuned). */
int hk_lq_solve_batch(hk_handle h, int batch, int N, const double* A, const double* B, const double* Q, const double* q,
                      const double* R, const double* x0, int horizon, double* u0_out);

/* device-resident variants used by bench.py / torch (pointers are HIP device pointers; stream = hipStream_t or NULL) */
int hk_lq_solve_batch_device(hk_handle h, int batch, int N, const double* dA, const double* dB, const double* dQ,
                             const double* dq, const double* dR, const double* dx0, int horizon, double* du0, void* stream);
/* The three state pointers below first settle the handle as any getter does (laggards of a lazily completed call, the completion guard of optimistic
 * short calls, a search launch on the planner's side stream — each may synchronise with the device), then return the buffer; NULL on failure
 * (hk_last_error).  What a pointer shows is complete once hk_stream has been synchronised; after further hk_step calls request it again. */
void* hk_device_results_ptr(hk_handle h);  /* hk_episode_result[E][A] on device: the payload of the RCCL all-gather */
void* hk_device_agents_ptr(hk_handle h);   /* hk_agent_state[E][A] on device: a SNAPSHOT as of this call (the library keeps the per-tick fields in a
                                            * wave-tiled layout of its own and gathers them into these records here, asynchronously on hk_stream;
                                            * write kart states with hk_set_agent_state, not through this pointer) */
/* Device-resident RL loop (an external trainer that keeps its tensors on the GPU): hk_observe runs CollectObservations into
 * the library's device buffer (asynchronous, on the handle's stream; raises the HitWall / HitOpponent reward events like
 * hk_get_observations); hk_rewards_device moves m_Reward / m_GroupReward into the two device buffers and zeroes the
 * accumulators (Agent.SendInfo); the trainer writes its actions straight into the action buffers before hk_step.
 * All four buffers are [E][A] (obs: [E][A][hk_obs_dim]); synchronise with hk_stream / hk_synchronize. */
int hk_observe(hk_handle h);
int hk_rewards_device(hk_handle h);
void* hk_device_obs_ptr(hk_handle h);           /* float[E][A][hk_obs_dim] */
void* hk_device_reward_ptr(hk_handle h);        /* float[E][A], valid after hk_rewards_device */
void* hk_device_group_reward_ptr(hk_handle h);  /* float[E][A], valid after hk_rewards_device */
void* hk_device_act_steer_ptr(hk_handle h);     /* float[E][A]: continuous action 0 */
void* hk_device_act_branch_ptr(hk_handle h);    /* int32[E][A]: discrete action 0 */
void* hk_stream(hk_handle h);              /* hipStream_t the handle launches on.  Short hk_step calls of a large plain handle leave half of the batch on a second
                                            * stream (joined lazily); this getter — like every entry point but hk_step — orders hk_stream behind it first, so work
                                            * a caller enqueues on the returned stream AFTER this call sees every tick issued so far.  Call it again after later
                                            * hk_step calls rather than caching the ordering (the handle itself never needs it: its own entry points join). */
/* What built this libhk.so (round 6): a JSON string compiled into the library at link time — hipcc / clang version, the flags, the hidden back-end switches the
 * toolchain accepted and, per translation unit, the code-generation guard variant it shipped with.  bench.py prints it in config.build. */
const char* hk_build_info(void);
/* The schedule the last hk_step of this handle ran (round 6; a JSON string owned by the handle, valid until the next hk_step): fixed / lazy / pause rounds,
 * fission or fused kernel, streams, the optimistic plan, where multi-player games are solved.  bench.py prints it in config.schedule. */
const char* hk_schedule_info(hk_handle h);
int hk_synchronize(hk_handle h);

/* ---- RL low-level policy inference on device ---------------------------------------------------------
 * Replaces the Barracuda execution of the ML-Agents 2.0.1 PPO actor that drives LowMode == RL agents
 * (BehaviorParameters.Model -> Agent.OnActionReceived KA:440 -> InterpretDiscreteActions HKA:1371-1379).  The network
 * is what mlagents-learn exports (the .onnx files under Assets/Karting/Prefabs/AI/, graph probed with
 * tools/onnx_read.py):  x = clip((obs - mean) / std, -5, 5);  n_layers x { x = swish(W x + b) };
 * mu = W_mu x + b_mu;  logits = W_br x + b_br;
 *   continuous_actions[0] = clip(mu + eps * exp(log_sigma), -3, 3) / 3,  eps ~ N(0,1)   (deterministic: eps = 0)
 *   discrete_actions[0]   ~ Categorical(softmax(logits))                                (deterministic: argmax)
 * obs = the agent's last `stack` CollectObservations vectors, oldest first, zero-filled after an episode reset
 * (ML-Agents StackingSensor).  A decision is taken on every tick t of the handle with t % decision_period == 0
 * (DecisionRequester, scene override DecisionPeriod = 2) and the action is repeated in between (TakeActionsBetweenDecisions).
 * Barracuda's random stream is not reproducible outside Unity: eps and the categorical draw come from Philox-4x32
 * keyed by `seed` (counter = decision index, row) instead — "parity unpinned" for the sampled outputs, exact for mu/logits.
 * All arithmetic is fp32: the GEMMs run on the f32-input MFMA, whose result is bit-for-bit a k-ascending fmaf chain
 * seeded with the bias, which is what the CPU oracle computes. */
#define HK_MAX_POLICIES 4
#define HK_POLICY_MAX_LAYERS 4
#define HK_POLICY_MAX_IN 1280     /* obs_dim * stack; HierarchicalKartAgent models: 216 (A = 2), 312 (A = 4), 624 (A = 4, stack 8) */
#define HK_POLICY_MAX_HIDDEN 256

typedef struct hk_policy_desc {
    int32_t in_dim;            /* obs_dim * stack; even */
    int32_t stack;             /* NumStackedVectorObservations (4) */
    int32_t hidden;            /* 32..256, multiple of 32 */
    int32_t n_layers;          /* 1..HK_POLICY_MAX_LAYERS */
    int32_t n_branch;          /* size of discrete branch 0 (3: brake / coast / accelerate) */
    int32_t normalize;         /* 1: apply (obs - mean) / std and the +-5 clip */
    int32_t deterministic;     /* 1: deterministic_continuous_actions / deterministic_discrete_actions */
    uint32_t seed;
    const float* norm_mean;    /* [in_dim] */
    const float* norm_std;     /* [in_dim] the exported divisor sqrt(variance / steps) */
    const float* W[HK_POLICY_MAX_LAYERS];  /* [hidden][k] row-major (torch Linear.weight); k = in_dim for layer 0, else hidden */
    const float* b[HK_POLICY_MAX_LAYERS];  /* [hidden] */
    const float* W_mu;         /* [hidden] */
    const float* b_mu;         /* [1] */
    const float* log_sigma;    /* [1] */
    const float* W_branch;     /* [n_branch][hidden] */
    const float* b_branch;     /* [n_branch] */
} hk_policy_desc;

/* Upload a policy and bind it to the agent slots listed (all must be LowMode == RL or E2E; hk_obs_dim * stack must equal
 * in_dim).  Returns the policy index (>= 0) or a negative hk_status.  decision_period (DecisionRequester) is per handle:
 * a second attach with a different period is refused with HK_ERR_INVALID. */
int hk_policy_attach(hk_handle h, const hk_policy_desc* desc, const int32_t* agent_slots, int n_slots, int decision_period);
/* PRECISION of an attached policy (hk_policy_set_precision; HK_POLICY_PREC_F32 is the default and is everything above, bit for bit with the
 * CPU oracle).  HK_POLICY_PREC_BF16 runs the policy's trunk on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16), operand for operand the
 * bf16 PPO trainer's forward (below, "PPO trainer" PRECISION): the input is normalised and clipped in fp32, then rounded once to bf16 (to
 * nearest even, Inf kept, a NaN becomes 0x7FC0); every trunk weight is rounded once from its fp32 value; each layer's fp32 accumulator is
 * seeded with the fp32 bias and stepped in ascending k over K zero-padded to a multiple of 64; the post-activations below the last layer are
 * rounded once to bf16, the last layer's stays fp32.  The heads, the arg-max, the sampling, both log-probabilities and the recorder's rows
 * are the fp32 tail of the default precision, unchanged, on that last activation.
 * What is given up: in HK_POLICY_PREC_BF16 the policy no longer agrees with the CPU oracle — mu / logits differ from it by the bf16 rounding
 * of the trunk, so actions, and therefore races, differ.  What is regained: with the trainer in HK_PPO_PREC_BF16 too, the training forward IS
 * the inference chain again, bit for bit, so at unchanged parameters rho == 1 and approx-KL and the clip fraction are exactly 0.  Mixed
 * settings (an fp32 trainer on a bf16 policy, or the reverse) are allowed and have the small non-zero statistics described there.
 * The precision is per policy and is set between calls; only hk_stream's order is implied.  The first switch to bf16 gives the policy a second
 * device allocation, the bf16 copies of its trunk weights in the matrix instruction's operand order, built on hk_stream from the CURRENT fp32
 * inference copies (so a switch after hk_ppo_publish is correct); hk_ppo_publish rebuilds them in the same call once they exist, each the
 * master weight rounded once (HK_PPO_SHADOW's element).  The fp32 copies are kept current in both modes: switching back to
 * HK_POLICY_PREC_F32 is the oracle's chain again, bit for bit.  Every consumer (hk_step's decisions of RL / MCTS-RL / E2E agents,
 * hk_policy_forward) follows the switch.  Refused with HK_ERR_INVALID and a message: a bad policy index, an unknown precision, and any switch
 * while a rollout is open (the rows of one rollout come from one chain); a refused call leaves the precision as it was.
 * hk_policy_get_precision: >= 0 the precision, < 0 an hk_status. */
typedef enum { HK_POLICY_PREC_F32 = 0, HK_POLICY_PREC_BF16 = 1 } hk_policy_precision;
int hk_policy_set_precision(hk_handle h, int policy, int precision);
int hk_policy_get_precision(hk_handle h, int policy);
/* The MLP alone on caller-supplied stacked observations (host pointers): mu[rows], logits[rows][n_branch]; in the policy's precision. */
int hk_policy_forward(hk_handle h, int policy, int rows, const float* obs /*[rows][in_dim]*/, float* mu, float* logits);
/* RECURRENT ACTORS: the ML-Agents NetworkBody with `memory: {memory_size, sequence_length}` (the reference's *-LSTM behaviours use
 * memory_size 256 on a 128 x 3 trunk).  With m = memory_size / 2 the actor is: normalise, the n x (Linear + Swish) of above giving a[hidden], ONE
 * LSTM cell, and the heads on h' (W_mu [m], W_branch [n_branch][m] in the hk_policy_desc given to hk_policy_attach_lstm):
 *   z_g[j] = b_g[j] + sum_k W_ih[g m + j][k] a[k]  (k = 0 .. hidden - 1 ascending)
 *                   + sum_k W_hh[g m + j][k] h[k]  (k = 0 .. m - 1 ascending, continuing the same fmaf chain)
 *            g in {i, f, g, o}, torch's order; b = fp32(b_ih + b_hh), summed once on the host at attach
 *   i = sigma(z_i)  f = sigma(z_f)  g~ = tanh(z_g)  o = sigma(z_o)      c' = fmaf(f, c, i g~)      h' = o tanh(c')
 *   mu = W_mu h' + b_mu     logits = W_branch h' + b_branch              (fmaf chains over m, ascending)
 * sigma and tanh are hk_sigmoidf / hk_tanhf_fast of csrc/hk_policy_lstm.h, fp32 on hk_expf_fast_core like the Swish; the gate products run on
 * v_mfma_f32_32x32x2_f32 with the accumulator seeded with b, bit for bit the chain written above.  A host build of the same functions
 * (tests/policy_lstm_host_check.cpp) reproduces mu, logits and the memory bit for bit.  Sampling, the clip, the arg-max, both
 * log-probabilities and the recorder's row are the fp32 tail of a plain actor, unchanged, applied to h'.
 * MEMORY of an (env, agent slot) is [h (m) | c (m)], hidden state first (ML-Agents' torch.cat([h, c])), fp32, kept in a device buffer of the
 * policy [E][n_slots][2m] indexed by LOGICAL env like the observation stack.  It is all zero at the first decision of an episode: the test is
 * the one that clears the stack (FIRST of the recorder), so hk_reset of some or all envs clears their memory at their next decision.
 *   hk_policy_attach_lstm    hk_policy_attach plus the cell.  A NULL lstm desc IS hk_policy_attach, launch for launch.
 *   hk_policy_memory_size    2m of the policy, 0 when it has no memory, < 0 an hk_status
 *   hk_policy_forward_mem    the actor alone on caller-supplied rows (host pointers): mem_in [rows][2m] (NULL: zeros) -> mu, logits and, when
 *                            mem_out is not NULL, the memory after the cell.  The policy's own memory is not touched.  Synchronises.
 *   hk_policy_memory_get     the policy's memory [E][n_slots][2m] to the host; synchronises
 *   hk_policy_memory_set     ... from the host.  What is set belongs to the episode each env is in NOW: the next decision keeps it (and does
 *                            not clear the observation stack) unless the episode changes first, which is what lets a race with a recurrent
 *                            actor resume on another handle after hk_set_agent_state / hk_set_env_state.
 *   hk_policy_memory_clear   hk_policy_memory_set of an all-zero array, on the device: a fill of [E][n_slots][2m] with +0.0 and the same epoch
 *                            words made current; asynchronous on hk_stream, no host round trip (a self-play driver that wants a swapped-in
 *                            opponent to start from a clean memory calls it after hk_policy_pool_load)
 * Refused with HK_ERR_INVALID, state as it was, hk_last_error naming the argument: memory_size odd; m not a multiple of 32 or outside
 * [32, 128]; a NULL weight pointer; reserved != 0; hk_policy_memory_set / _clear while a rollout is open; hk_policy_forward_mem, hk_policy_memory_get,
 * hk_policy_memory_set or _clear on a policy without memory or (the first three) with a NULL array.  Refused with HK_ERR_UNSUPPORTED on a policy WITH memory:
 * hk_policy_forward (use hk_policy_forward_mem), hk_policy_set_precision(HK_POLICY_PREC_BF16), hk_ppo_create (use hk_ppo_create_recurrent), hk_ppo_create_poca,
 * hk_policy_pool_create, and hk_policy_pool_save / _load with a feed-forward pool (use hk_policy_pool_create_recurrent: "SELF-PLAY" RECURRENT POOLS).
 * Training: hk_ppo_create_recurrent ("PPO trainer" RECURRENT).  Snapshot pools and opponent swaps: hk_policy_pool_create_recurrent.
 * bf16 for the trunk and the cell: hk_policy_lstm_set_precision (RECURRENT ACTORS IN BF16, below).  Out of scope: m above
 * 128, stacked or bidirectional LSTMs, and a CPU-oracle restatement (the bit reference is the host build named above). */
#define HK_POLICY_MAX_MEMORY 256          /* memory_size; m = memory_size / 2, a multiple of 32 in [32, 128] */
typedef struct hk_policy_lstm_desc {
    int32_t memory_size, reserved;
    const float *W_ih /*[4m][hidden]*/, *W_hh /*[4m][m]*/, *b_ih /*[4m]*/, *b_hh /*[4m]*/;   /* torch layout, gates i f g o */
} hk_policy_lstm_desc;
int hk_policy_attach_lstm(hk_handle h, const hk_policy_desc* desc, const hk_policy_lstm_desc* lstm, const int32_t* agent_slots, int n_slots, int decision_period);
int hk_policy_memory_size(hk_handle h, int policy);
int hk_policy_forward_mem(hk_handle h, int policy, int rows, const float* obs /*[rows][in_dim]*/, const float* mem_in /*[rows][2m], NULL: zeros*/,
                          float* mu, float* logits, float* mem_out /*[rows][2m] or NULL*/);
int hk_policy_memory_get(hk_handle h, int policy, float* mem /*[E][n_slots][2m]*/);
int hk_policy_memory_set(hk_handle h, int policy, const float* mem);
int hk_policy_memory_clear(hk_handle h, int policy);
/* RECURRENT ACTORS IN BF16 (hk_policy_lstm_set_precision for the policy, hk_ppo_recurrent_set_precision for its trainer; opt-in, the default and
 * every call above are untouched).  ONE chain, operand for operand, for inference and for the training forward:
 *   trunk   the bf16 chain of PRECISION above — input normalised in fp32 and rounded once, weights rounded once, the fp32 accumulator seeded
 *           with the fp32 bias and stepped by v_mfma_f32_32x32x16_bf16 in ascending k over K padded with +0.0 to whole chunks of 64 (the
 *           all-zero steps are issued), post-activations rounded once — with one difference: the LAST layer's post-activation a is rounded to
 *           bf16 too, because here it is an operand of the cell's product and no head reads it.
 *   gates   one fp32 accumulator per unit and gate (i, f, g, o), seeded with fp32(b_ih + b_hh), stepped in ascending k over a[0 .. hidden) with
 *           the padding steps of the 64-wide chunks (hidden = 32 or 96 is not a multiple of 64), then over h[0 .. m) in m / 16 whole steps.
 *           W_ih and W_hh are rounded once from the fp32 copies (in the trainer: the HK_PPO_SHADOW elements); h is rounded once where it is read
 *           as an operand.  The trainer stores Zx = bsum + a W_ih^T to fp32 between the two parts, which is lossless.
 *   cell    hk_lstm_cell, fp32 and unchanged.  c, c' and h' are fp32; the memory buffer, the recorder's MEMORY / NEXT_MEMORY rows and
 *           HK_PPO_MB_MEMORY stay fp32 [h | c]; where FIRST is set, h and c are exactly zero.
 *   heads   the heads, sampling, log-probabilities and the recorder's stores are the fp32 tail on the fp32 h'.
 *   trainer backward: both operands of every product the recurrent path adds are bf16 on the matrix cores with fp32 accumulation — the recurrent
 *           delta dG_tau W_hh, da = dG W_ih, dW_ih = dG^T a and dW_hh = dG^T h_prev.  Each operand is rounded once by the kernel that makes it
 *           (the cell backward rounds its gate deltas as it makes them, the step kernel stores the rounded h_prev).  A bias gradient is the fp64
 *           column sum of the rounded gate deltas.  Masters, GRAD, the Adam moments, dc, the cell backward itself, dh' from the heads and the head
 *           weight gradients stay fp32.  No float atomics: the same call on the same state gives the same bits.
 * Given up while the mode is on: agreement with the host twin of the fp32 chain.  Switching back restores it bit for bit.  With policy and
 * trainer both in bf16 the training forward IS the inference chain: rho == 1, approx-KL == clip fraction == 0 at unchanged parameters; mixed
 * settings are allowed and give small non-zero statistics, as for plain actors.
 *   hk_policy_lstm_set_precision   for a policy WITH memory (one without: HK_ERR_INVALID, use hk_policy_set_precision).  Refused with
 *                            HK_ERR_INVALID while a rollout is open, for an unknown precision or a bad index; a refused call leaves the precision
 *                            as it was.  The first switch to bf16 builds the bf16 copies of the trunk layers and of W_ih / W_hh in the matrix
 *                            instruction's operand order on hk_stream from the CURRENT fp32 copies; hk_ppo_publish of a recurrent trainer and
 *                            hk_policy_pool_load from a recurrent pool rebuild them in the same call.  hk_policy_get_precision reports it.
 *   hk_ppo_recurrent_set_precision ("PPO trainer" RECURRENT)  hk_ppo_set_precision for a trainer made by hk_ppo_create_recurrent; its MLP critic
 *                            goes on the bf16 trunk path.  A trainer with a recurrent critic: HK_ERR_UNSUPPORTED, state as it was (the critic's
 *                            cell stays fp32).  Any other trainer: HK_ERR_INVALID (use hk_ppo_set_precision).  hk_ppo_get_precision reports it.
 *   hk_ppo_lstm_gates_bf16   a debug tap in the spirit of hk_ppo_gemm_bf16, on raw bf16 bit patterns in the caller's DEVICE buffers: the trainer's
 *                            own two launches — the Zx product, then one step kernel's gate chains without the cell — returning the fp32
 *                            pre-activations z [rows][4m].  a [rows][H], h [rows][m], W_ih [4m][H], W_hh [4m][m] (torch layout), bsum [4m] fp32.
 *                            HK_ERR_INVALID: a NULL operand, non-positive sizes, H or m not a multiple of 32.  Asynchronous on hk_stream.
 * Out of scope: bf16 for a recurrent critic's cell, bf16 memory or recorder rows, m above 128. */
int hk_policy_lstm_set_precision(hk_handle h, int policy, int precision);
int hk_ppo_recurrent_set_precision(hk_handle h, int trainer, int precision);
int hk_ppo_lstm_gates_bf16(hk_handle h, int rows, int H, int m, const void* a_dev, const void* h_dev, const void* W_ih_dev, const void* W_hh_dev,
                           const float* bsum_dev, float* z_dev);
/* The actions currently latched for every agent (what the policies / hk_set_actions wrote): steer[E][A], branch[E][A] */
int hk_get_actions(hk_handle h, float* steer, int32_t* branch);

/* ---- rollout recorder: what the attached actors did, gathered on the device ---------------------------------------------
 * While a rollout is open, decision t (the t-th since hk_rollout_begin) writes ROW t of library-owned device buffers, and the
 * ticks that follow it up to the next decision (interval t) complete the row's rewards and done flag.  Recording changes no
 * result bit of the simulation.  Layouts are [R][E][A] (R = the rows given to hk_rollout_begin) unless noted; entries of agent
 * slots no actor drives stay 0.  Every field is 4 bytes per element (f32 or i32).
 *   OBS [R][E][A][obs_dim]     the observation decision t pushed into the agent's stack (the newest slice)
 *   FIRST i32                  1: the stack was cleared at decision t (first decision of an episode, or after a reset)
 *   STEER f32, BRANCH i32      the actions latched at decision t (what hk_get_actions returns after it)
 *   RAW f32                    the continuous sample before the clip, mu + eps * sigma: STEER == clip(RAW, -3, 3) / 3; RAW == MU when deterministic
 *   MU f32, LOGITS f32 [R][E][A][n_branch_max]    the actor's heads
 *   LOGP_CONT, LOGP_DISC f32   -0.5 ((RAW - mu) / sigma)^2 - log_sigma - 0.5 log(2 pi) and log_softmax(logits)[BRANCH] (ML-Agents: the
 *                              log-probability of the UNCLIPPED sample, continuous and discrete kept apart)
 *   REWARD, GROUP_REWARD f32   m_Reward / m_GroupReward moved out (and zeroed) at the end of interval t: what hk_get_rewards would return
 *                              then.  That includes the HitWall / HitOpponent events decision t's CollectObservations raised (ML-Agents would
 *                              count them toward the row before).  If an episode ended inside the interval: only the part after the reset.
 *   TERM_REWARD, TERM_GROUP_REWARD f32   an episode ended inside interval t: m_Reward / m_GroupReward at ResetGame, after the goal-timing
 *                              rewards, just before they are zeroed (what EndGroupEpisode sends); 0 otherwise and without hk_config.rewards
 *   DONE i32 [R][E]            0, 1 (an episode ended inside interval t) or 2 (... by the time-out)
 *   RING0 f32 [E][A][stack_max - 1][obs_dim]   the stack contents before decision 0, oldest first, right-aligned (an actor of stack s uses
 *                              the last s - 1 entries; zeros where empty): with OBS and FIRST every stacked input of the rollout can be rebuilt
 *   NEXT_OBS f32 [E][A][obs_dim]   written by hk_rollout_close: the observation of the decision after the last row (bootstrap input)
 *   MEMORY f32 [R][E][A][mem_max]   recurrent actors ("RECURRENT ACTORS" above) only: the memory [h | c] decision t READ, after the episode
 *                              zeroing and before the cell; mem_max = the largest 2m of the handle's actors, entries of slots whose actor has
 *                              none stay 0.  A row is self-contained: MU / LOGITS of row t follow from its stacked input and MEMORY[t] alone,
 *                              MEMORY[t + 1] is the cell's output at row t unless FIRST[t + 1], and MEMORY[t] == 0 exactly where FIRST[t] == 1.
 *                              4 * 2m bytes per row and agent (1 KiB at m = 128: 3.3 x the OBS row of obs_dim 78).
 *   NEXT_MEMORY f32 [E][A][mem_max]   written by hk_rollout_close beside NEXT_OBS: the memory after the last completed row, zero where
 *                              DONE of that row != 0 (the bootstrap memory)
 *                              On a handle without a recurrent actor both have no elements: hk_rollout_ptr returns NULL for them (with a
 *                              message), nothing is allocated for them and no launch is added.
 * A trainer's transition reward of row t is DONE ? TERM_REWARD : REWARD; TERM_REWARD + REWARD is every AddReward of the interval.
 * hk_rollout_begin allocates (or reuses) and zeroes the buffers, snapshots RING0 and the episode counters.  Refused (HK_ERR_INVALID):
 * no actor attached, a rollout already open, the Academy step not on a decision (a multiple of decision_period), rows < 1;
 * HK_ERR_UNSUPPORTED with hk_config.auto_reset == 0 (an ended episode is parked, never reset).  While a rollout is open an hk_step that
 * would take more decisions than rows remain is refused before anything is issued, and hk_reset, hk_set_agent_state, hk_set_env_state,
 * hk_get_rewards, hk_rewards_device and hk_policy_attach are refused (the two reward reads would take the accumulators the rows are made of).
 * hk_rollout_close is refused mid-interval; it writes NEXT_OBS with an observe launch that raises no reward events (the next decision
 * raises them as usual) and fails (HK_ERR_INVALID; the rollout is closed all the same) if an env ended more than one episode inside one
 * interval, which the rows cannot express.  The buffers stay readable until the next hk_rollout_begin or hk_destroy.  Everything is
 * asynchronous on hk_stream: synchronise before reading. */
typedef enum hk_rollout_field {
    HK_RO_OBS = 0, HK_RO_FIRST, HK_RO_STEER, HK_RO_BRANCH, HK_RO_RAW, HK_RO_MU, HK_RO_LOGITS, HK_RO_LOGP_CONT, HK_RO_LOGP_DISC,
    HK_RO_REWARD, HK_RO_GROUP_REWARD, HK_RO_TERM_REWARD, HK_RO_TERM_GROUP_REWARD, HK_RO_DONE, HK_RO_RING0, HK_RO_NEXT_OBS,
    HK_RO_MEMORY, HK_RO_NEXT_MEMORY,
    HK_RO_FIELDS
} hk_rollout_field;
int hk_rollout_begin(hk_handle h, int rows);
int hk_rollout_rows(hk_handle h);               /* completed rows: decisions whose interval has fully been issued */
int hk_rollout_close(hk_handle h);
void* hk_rollout_ptr(hk_handle h, int field);   /* device pointer of an HK_RO_* field; NULL (hk_last_error) on a bad field or before any rollout */

/* ---- PPO trainer: train an attached actor on a closed rollout, on the device ----------------------------------------------
 * One trainer per hk_ppo_create: an attached actor (policy), a critic of its own and Adam over both; it allocates nothing before hk_ppo_create.
 * ROWS: the trainer of policy p trains on the rows (t, e, j), t < R, e < E, j = the j-th of p's agent_slots, flattened in that order:
 * row id = (t E + e) S + j, n = R E S, where R is the number of COMPLETED rows (hk_rollout_rows at hk_rollout_close; a rollout may close
 * before all the rows hk_rollout_begin allotted, and the rest are never read).  The input of a row is the stacked input the actor saw there, rebuilt on the device from OBS, FIRST
 * and RING0 by the rule of rollout.stacked_inputs (never materialised for the whole rollout); the bootstrap input of (e, j) is the last row's
 * stack shifted by one with NEXT_OBS pushed (NEXT_OBS is the decision after the last completed row; unused where DONE[R - 1] != 0).
 * CRITIC: n_layers x (Linear + Swish) on the actor's normalised, clipped input (the actor's normaliser), then one linear output; initial
 * weights from an hk_policy_desc (W[], b[] the trunk, W_mu / b_mu the value head, n_branch = 0, in_dim = the actor's; hidden / n_layers
 * within the actor's limits, other fields ignored).  It shares no weight with the actor (ML-Agents shared_critic: false).
 * REWARD, DONE: r_t = DONE ? TERM_REWARD : REWARD (rollout.transition_rewards); every DONE != 0, the time-out (2) included, is terminal.
 * GROUP_REWARD is not used: PPO ignores group rewards (a POCA trainer, "POCA" below, is what reads them).
 * GAE per (e, j), backwards over t, V = V_OLD (the critic at hk_ppo_advantages), V_R = the bootstrap value, A_R = 0:
 *   delta_t = r_t + gamma (1 - d_t) V_{t+1} - V_t;   A_t = delta_t + gamma lambd (1 - d_t) A_{t+1};   RET_t = A_t + V_t
 * normalize_advantages: ADV = (A - mean) / (std + 1e-10) over all n rows (population std; mean and std in fp64, fixed order); RET keeps A unnormalised.
 * LOSS over a minibatch of m valid rows, new heads mu, logits, value v; logp_c / logp_d exactly as the recorder computes LOGP_CONT of RAW and
 * LOGP_DISC of BRANCH (so unchanged parameters give rho == 1 bit for bit):
 *   rho_c = exp(logp_c - LOGP_CONT), rho_d = exp(logp_d - LOGP_DISC)
 *   L_pi = -mean over rows and {c, d} of min(rho A, clip(rho, 1 - eps, 1 + eps) A)          (ML-Agents' per-column trust region)
 *   L_v  = mean max((RET - v)^2, (RET - V_OLD - clip(v - V_OLD, -eps, eps))^2)
 *   H    = 0.5 log(2 pi e) + log_sigma - sum softmax log_softmax
 *   L    = L_pi + 0.5 L_v - beta mean H
 * Gradients follow torch's conventions at ties: min / max split the gradient evenly, clip passes it inside [lo, hi] inclusive.
 * Departure from ML-Agents: no 1e-7 inside the log-probabilities and the entropy (the recorder has none either).
 * ADAM over the actor's and the critic's parameters (never the normaliser: NORMALISER below), step s = 1, 2, ... counted per trainer, in fp32, in this order:
 *   m = b1 m + (1 - b1) g;  v = b2 v + ((1 - b2) g) g;  p = p - lr (m / c1) / (sqrt(v / c2) + eps)
 * with (1 - b1), (1 - b2) rounded to fp32 once, c1 = 1 - b1^s and c2 = 1 - b2^s evaluated in fp64 and rounded to fp32; every operation
 * rounded to fp32 (no fused multiply-add), sqrt and division correctly rounded.
 * PARAMS / GRAD / ADAM_M / ADAM_V: one flat fp32 vector, torch layout (W [out][in]): the actor's W[0], b[0], W[1], b[1], ..., W_mu [H], b_mu [1],
 * log_sigma [1], W_branch [n_branch][H], b_branch [n_branch], then the critic's W[0], b[0], ..., W_v [Hc], b_v [1].
 * ENTRY POINTS (HK_ERR_INVALID with hk_last_error on: a bad trainer index or field; a rollout that is open, never opened, closed with no
 * completed row, or that began before
 * the policy was attached; a trainer whose hk_ppo_advantages ran on an earlier rollout than the current one, for minibatch / update; a critic
 * whose in_dim or limits do not fit; publish while a rollout is open):
 *   hk_ppo_create      -> trainer index.  Copies the actor's parameters as attached into the master copy; cfg NULL: the defaults below.
 *   hk_ppo_advantages  the critic over the n rows and the E S bootstrap inputs, then GAE: V_OLD, ADV, RET [n].
 *   hk_ppo_minibatch   the loss of the rows rows_dev[0 .. m) (a device pointer) and its gradient into GRAD.  An id outside [0, n) is skipped
 *                      (counted in the stats, never read).  stats (host, [HK_PPO_STATS], NULL: none; non-NULL synchronises):
 *                      L_pi, L_v, mean H, approx-KL (mean over rows and {c, d} of old - new logp), clip fraction (of rows x {c, d}), skipped rows.
 *   hk_ppo_adam        one Adam step from GRAD.
 *   hk_ppo_update      epochs x (a permutation of the n rows generated on the device, keyed by the shuffle seed and the trainer's epoch count;
 *                      floor(n / minibatch) minibatches (one of n rows when n < minibatch), each hk_ppo_minibatch + hk_ppo_adam), then
 *                      hk_ppo_publish.  stats: the mean over the last epoch's minibatches.
 *   hk_ppo_publish     re-lays the master actor parameters into the attached policy's inference copies (what hk_policy_attach builds).
 *   hk_ppo_ptr / hk_ppo_count   device pointer / element count of an HK_PPO_* field.  MB_MU, MB_LOGITS [m][n_branch], MB_VALUE: the heads and
 *                      the value of the last minibatch's rows (a debug tap).  PERM (int32 [n]): the row permutation of the last epoch of the last
 *                      hk_ppo_update on the current advantages (the k-th epoch of a trainer, k = 0, 1, ..., is keyed by (seed, k)).
 * Row ids of hk_ppo_minibatch are read on hk_stream: a caller that writes them on another stream orders the two first (PPOTrainer does).
 * PRECISION (hk_ppo_set_precision; HK_PPO_PREC_F32 is the default and is everything above, bit for bit).  HK_PPO_PREC_BF16 is mixed precision
 * with fp32 master weights: both operands of every TRUNK matrix product of the actor and the critic — the forward a_l = swish(W_l a_{l-1} + b_l),
 * the backward delta (delta W_l) * swish' and the weight gradient delta^T a_{l-1}, in hk_ppo_advantages as in a minibatch — are bf16, multiplied
 * on the bf16 matrix cores and accumulated in fp32 (the forward accumulator seeded with the fp32 bias).  Each operand is rounded ONCE, where it is
 * made, to nearest even (Inf kept, a NaN becomes the quiet NaN 0x7FC0): the trunk weights into a bf16 shadow of PARAMS (HK_PPO_SHADOW) after
 * every Adam step, when the mode is switched on and at the entry of hk_ppo_advantages / hk_ppo_minibatch / hk_ppo_update (PARAMS is writable); the normalised,
 * clipped input by the gather; the post-activations below the last layer and every delta by the kernel that makes them (so a bias gradient is
 * the fp64 column sum of the rounded deltas).  Everything else stays fp32 and is computed as above: PARAMS, GRAD, the Adam moments, V_OLD / ADV /
 * RET, the pre-activations swish' reads, the last layer's post-activation and the heads, log-probabilities, losses and per-row gradients on
 * it, the head weight gradients, the column sums (fp64), the split-K combine (chunks of 256 rows, in chunk order) and hk_ppo_publish, which
 * copies the fp32 masters (and rebuilds a bf16 policy's weight copies from them, equal to the shadow element for element).  No float atomics: the same call on the same state gives the same bits.
 * What is no longer exact while the POLICY stays in HK_POLICY_PREC_F32 (in HK_POLICY_PREC_BF16 the two chains are one again, see there): the
 * training forward is not the inference chain, and the rollout's LOGP_* come from the fp32 inference chain, so
 * at unchanged parameters rho != 1, approx-KL and the clip fraction are small non-zero numbers and MB_MU / MB_LOGITS differ from MU / LOGITS
 * by the bf16 rounding of the trunk.  Switching back to HK_PPO_PREC_F32 restores the exact path.  The precision is set between calls (a call
 * waits for hk_stream and releases the minibatch workspace, which is laid out per precision: MB_* are unavailable until the next minibatch);
 * an unknown value or a bad trainer index is refused with HK_ERR_INVALID.
 * hk_ppo_gemm_bf16 (a debug tap in the spirit of hk_policy_forward) runs ONE product of the bf16 kernel on the caller's device buffers, bf16
 * operands as raw 16-bit patterns, C fp32 [M][N], on hk_stream: epi 1 (forward) C = swish(bias + A B^T), A [M][K], B [N][K], bias [N] or NULL;
 * epi 2 (backward delta) C = (A B) * swish'(aux), A [M][K], B [K][N], aux fp32 [M][N]; epi 0 (weight gradient) C = A^T B, A [K][M], B [K][N],
 * split over K in chunks of 256 and combined in chunk order (synchronises).  A NULL operand, a non-positive M / N / K or another epi is refused.
 * NORMALISER (hk_ppo_normalizer_*; opt-in: a trainer that never calls them leaves the statistics frozen as attached, and every entry point above
 * computes what it computed, bit for bit).  STATE per trainer, once initialised: a step count N (int64) and, per stacked input k < in_dim, an
 * fp64 mean m_k and an fp64 sum of squared deviations M2_k — ML-Agents' normalization_steps, running_mean and running_variance, kept in fp64.
 * The attached policy's fp32 statistics are the PUBLISHED form, mean_k = fp32(m_k), std_k = fp32(sqrt(M2_k / N)) with the division and the square
 * root in fp64 (correctly rounded): hk_policy_desc.norm_std's exported divisor.  They live where hk_policy_attach put them and are read in place by
 * both inference chains (fp32 and bf16) and by the trainer's gather, so every consumer follows a publication; clip((x - mean) / std, -5, 5) is untouched.
 *   hk_ppo_normalizer_init    N = steps (>= 1), m_k = mean_k, M2_k = (double)std_k^2 * steps from the policy's CURRENT device values (synchronises;
 *                             publishes nothing).  A fresh actor attached with mean 0, std 1 and steps = 1 is ML-Agents' initial normaliser.
 *   hk_ppo_normalizer_update  folds the trainer's n = R E S rows of the closed rollout (its COMPLETED rows; the preconditions of hk_ppo_advantages)
 *                             into the state and publishes.  x_ik is the UN-normalised stacked input of row i, rebuilt by the rule of ROWS above
 *                             (an absent entry is 0 and counts, as ML-Agents' zero-padded stack does; the bootstrap rows are excluded).  With
 *                             c_ik = x_ik - m_k:  N' = N + n;  delta_k = sum_i c_ik;  m'_k = m_k + delta_k / N';
 *                             M2'_k = M2_k + sum_i (x_ik - m'_k)(x_ik - m_k), evaluated in one pass as sum_i c_ik^2 - delta_k^2 / N' — ML-Agents'
 *                             batch update, algebraically independent of how the rows are split into batches.  All sums are fp64 over a partition
 *                             of the recorded observations fixed by the shapes, combined in partition order; no float atomics: the same call on
 *                             the same state gives the same bits.  Asynchronous.
 *   hk_ppo_normalizer_get     steps, mean [in_dim], m2 [in_dim] to host pointers (any may be NULL); synchronises.
 *   hk_ppo_normalizer_set     loads a state (host pointers) and publishes it; with get, the normaliser's checkpoint.  Synchronises.
 * Refused with HK_ERR_INVALID (state and published values as they were): every one of the four on a policy attached with normalize == 0 (it has
 * no buffers) or while a rollout is open (the rows of one rollout come from one chain); init / set on steps < 1, a non-finite mean, a std (init)
 * or m2 (set) that is not finite and > 0, set on a NULL array; update / get before init or set; update on whatever hk_ppo_advantages refuses.
 * After update or set the advantages of EVERY trainer of that policy are stale (V_OLD is the critic on inputs it will not be trained on):
 * hk_ppo_minibatch / hk_ppo_update are refused until hk_ppo_advantages has run again, exactly as after a new rollout.
 * ORDER (neither is enforced).  ML-Agents' order, normalizer_update -> advantages -> update: the rollout's LOGP_* were recorded under the old
 * statistics, so rho != 1 at unchanged parameters.  The exact order, advantages -> update -> normalizer_update: the new statistics act from the
 * next rollout on, rho == 1 and the bit-equal training forward hold as above, in both precisions.  A dimension that never varies keeps M2_k at its
 * initial value, so its std shrinks as 1 / sqrt(N): ML-Agents' behaviour, not guarded.
 * HK_PPO_NORM_MEAN / HK_PPO_NORM_STD (hk_ppo_ptr): the policy's published fp32 statistics themselves, [in_dim]; count 0 on normalize == 0.
 * LONG RUNS (hk_ppo_update_opt, hk_ppo_adam_clipped, hk_ppo_get_counters / hk_ppo_set_counters; opt-in: a trainer that never calls them computes
 * what it computed, bit for bit, and allocates nothing more).  Neither clipping nor the KL stop is in ML-Agents' PPO; both are additions.
 * CLIP by the global L2 norm of the whole flat GRAD vector, actor and critic together (one optimiser, one norm: torch's clip_grad_norm_ over
 * all parameters), computed on the device:
 *   norm2 = sum_i (double)g_i (double)g_i in fp64 (a square of an fp32 value is exact in fp64; the only error is the fp64 additions), over a
 *   partition of GRAD into runs of 4096 elements and in an order both fixed by P alone, no atomics: the same call on the same state gives the
 *   same bits;  norm = sqrt(norm2) in fp64, correctly rounded;  coef = (float) min(1.0, (double)max_grad_norm / (norm + 1e-6)), rounded to fp32
 *   once (torch's clip_coef and clamp).  The step is ADAM above, operation for operation, on g'_i = g_i * coef (one fp32 multiply, rounded, no
 *   fused multiply-add); GRAD itself stays as the minibatch wrote it.  With coef == 1.0f the multiply is exact: max_grad_norm = +inf ("measure
 *   only") and any bound above the norm give exactly the bits of the plain step.
 * NON-FINITE GRADIENT: when norm2 is not finite (a NaN or an Inf anywhere in GRAD) the step writes nothing — PARAMS, ADAM_M and ADAM_V keep their
 * bits — and is counted in CLIP[4]; CLIP[1] is then 0.  Documented departure: the step count s still advances (the host cannot know without a
 * synchronise), so the bias corrections of the following steps are those of one step more.
 * HK_PPO_CLIP (hk_ppo_ptr; fp64 [8]; count 0 before the first clip-aware step has allocated it): [0] norm and [1] coef (the fp32 value widened) of
 * the last clip-aware step; [2] steps taken, [3] steps with coef < 1, [4] non-finite steps, [5] the sum and [6] the maximum of norm over the finite
 * steps; [7] reserved, 0.  [2 .. 6] accumulate: zero at hk_ppo_create and zeroed, stream-ordered, at the entry of hk_ppo_update_opt.
 *   hk_ppo_adam_clipped  one clip-aware step from GRAD; max_grad_norm > 0 (+inf allowed), anything else — 0, a negative, a NaN — is refused.
 *   hk_ppo_update_opt    hk_ppo_update's loop (they share it) with two options; with both 0 the launches issued are exactly hk_ppo_update's.
 *                        max_grad_norm > 0: every step is the clip-aware one.  target_kl > 0, the KL STOP: the stats accumulator is zeroed at the
 *                        start of every epoch and read after its last step (one 64-byte copy and a synchronise per epoch, only in this mode); if
 *                        that epoch's mean approx-KL is > target_kl no further epoch runs.  stats is then that epoch's mean, the epoch count has
 *                        advanced by the epochs actually run (the next update's permutation key follows on), PERM is the last epoch run, and
 *                        hk_ppo_publish happens as usual.  The first epoch always runs.  Per epoch, not per minibatch, on purpose: a read per
 *                        minibatch would serialise the launch-bound small-minibatch update.
 *                        report (or NULL; non-NULL synchronises): epochs_run, minibatches_run, stopped_by_kl; clipped_steps, nonfinite_steps,
 *                        grad_norm_mean (over the finite steps) and grad_norm_max of this call from CLIP (0 with clipping off); last_epoch_kl,
 *                        stats[3] in fp64 before rounding.
 *   hk_ppo_get_counters / hk_ppo_set_counters   the Adam step count s (it gives c1, c2) and the epoch count k (it keys the shuffle as (seed, k)):
 *                        the missing piece of RESUME.  A caller restores PARAMS / ADAM_M / ADAM_V through hk_ppo_ptr, the normaliser through
 *                        hk_ppo_normalizer_set, and these two words; a trainer restored so and fed the same rollout continues bit for bit.  set
 *                        takes 0 <= each <= INT32_MAX, is refused while a rollout is open (as hk_ppo_publish is) and leaves the advantages as
 *                        valid as they were.  Either pointer of get may be NULL.
 * Refused with HK_ERR_INVALID and a message naming the argument, state as it was: a NULL opts, epochs < 1, minibatch < 1, max_grad_norm or target_kl
 * negative or NaN, target_kl infinite, reserved != 0, and whatever hk_ppo_update / hk_ppo_adam refuse.
 * RECURRENT (hk_ppo_create_recurrent: PPO with truncated back-propagation through time for an actor with memory, "RECURRENT ACTORS" above; the
 * reference's *-LSTM behaviours train with memory_size 256, sequence_length 64).  It returns a trainer index of the same table and every hk_ppo_*
 * entry point takes it; a trainer made by hk_ppo_create or hk_ppo_create_poca computes what it computed, bit for bit, issues the launches it issued
 * and allocates nothing more.  hk_ppo_create itself keeps refusing a policy with memory (HK_ERR_UNSUPPORTED), hk_ppo_config is as it was.
 * The CRITIC of a trainer made by hk_ppo_create_recurrent stays the feed-forward critic above on the stacked input, so its hk_ppo_advantages,
 * GAE and V_OLD are those of a plain trainer; ML-Agents gives the critic an LSTM of its own: hk_ppo_create_recurrent_critic, RECURRENT CRITIC below.
 * SEQUENCES.  With L = sequence_length and R the completed rows, window k of agent (e, j) is the rows t in [k L, min((k + 1) L, R)); sequence id
 * s = (k E + e) S + j, n_seq = ceil(R / L) E S.  The memory entering a window's first row is the recorder's MEMORY[k L], a constant: no gradient
 * flows into it.  Inside a window the training forward carries the memory itself.  At a row with FIRST[t] == 1 the memory read is exactly zero
 * and no gradient crosses that row backwards (gradients still flow within the row).  The rows tau of the last window with k L + tau >= R are
 * dead: exact zeros in every loss term, delta and gradient contribution, like a skipped id.
 * MINIBATCHES.  As for POCA's group ids, an id handed to hk_ppo_minibatch is a SEQUENCE id and m counts sequences; an id outside [0, n_seq) skips
 * its sequence and stats[5] counts skipped sequences.  Under hk_ppo_update / hk_ppo_update_opt `minibatch` counts sequences, the permutation is
 * over n_seq and PERM is int32 [n_seq].  Loss means are over the valid rows, as above.  The rows are gathered time-major: MB_MU, MB_LOGITS and
 * MB_VALUE are [L][m], and HK_PPO_MB_MEMORY [L][m][2 m_cell] holds the memory [h' | c'] each row's cell wrote.
 * PARAMS / GRAD / ADAM_M / ADAM_V, actor part: the trunk as above; then W_ih [4 m_cell][H], W_hh [4 m_cell][m_cell], b_ih [4 m_cell],
 * b_hh [4 m_cell] in torch layout, gates i f g o; then the heads, m_cell wide; then the critic, unchanged.  The gate bias the forward uses is
 * fp32(b_ih + b_hh), formed as at attach; both biases receive the same gradient.
 * EXACTNESS.  A gate pre-activation is the inference chain: seeded with the summed bias, one ascending-k fmaf chain over a[0 .. H), then over
 * h[0 .. m_cell), on v_mfma_f32_32x32x2_f32 (the partial chain is stored to fp32 memory between the two parts, which is lossless); the cell is
 * hk_lstm_cell, the heads fmaf chains on h'.  At unchanged parameters in the exact order (advantages -> update -> normaliser): rho == 1, approx-KL
 * and the clip fraction exactly 0, MB_MU / MB_LOGITS equal to the recorder's MU / LOGITS bit for bit, MB_MEMORY at row t equal to MEMORY[t + 1]
 * wherever FIRST[t + 1] == 0 and to NEXT_MEMORY at the last row where DONE == 0.
 * BACKWARD.  sigma' = s (1 - s) and tanh' = 1 - t^2 from the stored gate outputs.  With dh_tau the heads' delta at tau plus the recurrent delta
 * from tau + 1, the cell backward gives the four gate deltas dG_tau and dc_{tau-1}; the recurrent delta to tau - 1 is dG_tau W_hh, zeroed (with dc)
 * where FIRST of row tau is set, and at tau = 0.  Over all rows of the minibatch at once, in the fixed-order split-K forms above (chunks of 256 rows,
 * combined in chunk order; no float atomics: the same call on the same state gives the same bits): dW_ih = dG^T a, dW_hh = dG^T h_prev (h_prev as
 * read, after the reset), db = the fp64 column sum of dG, da = (dG W_ih) * swish'(Z_last), handed to the trunk's backward.
 * hk_ppo_adam / hk_ppo_adam_clipped (one norm over everything, the cell included), hk_ppo_update(_opt) with clip and KL stop, the counters, the
 * normaliser (it acts on inputs) and hk_ppo_ptr / hk_ppo_count work without a change of meaning.  hk_ppo_publish also rewrites the policy's
 * group-major Wq_ih / Wq_hh copies and the summed bias.
 * Refused with HK_ERR_INVALID, state as it was, the message naming the argument: a NULL r, sequence_length < 1, reserved != 0, a policy without
 * memory (use hk_ppo_create) and whatever hk_ppo_create refuses.  HK_ERR_UNSUPPORTED: hk_ppo_set_precision(HK_PPO_PREC_BF16) on a recurrent trainer.
 * RECURRENT CRITIC (hk_ppo_create_recurrent_critic: the recurrent trainer above whose critic has an LSTM cell of its own, as ML-Agents' ValueNetwork
 * built from the actor's network_settings; the reference's *-LSTM behaviours trained so).  Everything above holds for the actor side, unchanged;
 * a trainer made by hk_ppo_create, hk_ppo_create_recurrent or hk_ppo_create_poca computes what it computed, bit for bit, issues the launches it
 * issued and allocates nothing more.
 * CRITIC.  The actor's normalised, clipped stacked input (the ACTOR's normaliser) -> n_layers x (Linear + Swish) of width Hc -> ONE LSTM cell of
 * m_v = critic_cell.memory_size / 2 units (a multiple of 32 in [32, 128], gates i f g o) -> v = b_v + sum_k W_v[k] h'[k].  Its arithmetic is a
 * recurrent actor's, bit for bit: a gate pre-activation is the fmaf chain seeded with fp32(b_ih + b_hh), ascending over a[0 .. Hc), then over
 * h[0 .. m_v), on v_mfma_f32_32x32x2_f32; the cell is hk_lstm_cell; the value head is the ascending fmaf chain of the actor's mu head.  EXACTNESS:
 * a recurrent POLICY whose trunk, cell and W_mu / b_mu are the critic's trunk, cell and W_v / b_v and whose normaliser is the actor's returns,
 * through hk_policy_forward_mem, a mu that is V_OLD bit for bit.
 * CRITIC MEMORY.  [h | c], 2 m_v floats per (e, j).  At a row with FIRST[t] == 1 the memory read is exactly zero (the actor's rule).  At row 0 of
 * a rollout the memory read is HK_PPO_CRITIC_MEM_IN[e][j], subject to the FIRST rule; it is all zero at create.  The first hk_ppo_advantages on
 * a rollout generation the trainer has not seen sets MEM_IN := MEM_OUT of its previous call (zero before any), then runs; a repeated call on
 * the same rollout (after hk_ppo_normalizer_update, say) re-uses MEM_IN unchanged and gives the same bits.  HK_PPO_CRITIC_MEM_OUT is the memory
 * after row R - 1, zero where DONE[R - 1] != 0.  Both are writable through hk_ppo_ptr, as PARAMS is: writing MEM_IN acts on the next call on
 * the SAME rollout, writing MEM_OUT on the first call on the next one.  This is ML-Agents' critic_memory_dict: it is carried whatever happened
 * between the rollouts (a reset, other steps), and it goes stale under parameter updates — it was computed by the parameters of the pass that
 * wrote it, and is not recomputed.
 * VALUE PASS.  hk_ppo_advantages runs the critic sequentially: for every (e, j), in time order t = 0 .. R - 1, one critic step per row gives
 * V_OLD[t]; one more step on the bootstrap input (NEXT_OBS pushed into the stack) from the memory after row R - 1 gives the bootstrap value,
 * unused where DONE[R - 1].  GAE and the advantage normalisation run exactly as for a plain trainer.  It records HK_PPO_CRITIC_MEMORY
 * [ceil(R / L)][E][S][2 m_v]: the memory carried INTO row k L, before the FIRST rule (the training forward applies that rule itself) — the critic's
 * twin of the recorder's MEMORY[k L].  The steps go value_chunk_steps at a time per launch (0: the default, 16) over tiles of sequences; the
 * result depends on neither, bit for bit.
 * TRAINING.  Windows, sequence ids, the time-major gather, dead rows and the skipped-id rule are those above.  The critic's forward over a window
 * starts from CRITIC_MEMORY[k], a constant (no gradient flows into it), carries the memory itself and zeroes it at FIRST, in value and in
 * gradient; the loss reads the critic's h' (m_v wide) under W_v.  The backward is BACKWARD above applied to the critic: the value-head delta
 * onto h', the cell backward L times in reverse with the recurrent-delta product, dW_ih, dW_hh and the two biases (the same gradient) over all
 * rows at once in the fixed-order split-K forms, da into the critic's trunk.  No float atomics.  At unchanged parameters: MB_VALUE == V_OLD bit
 * for bit on every live row; HK_PPO_MB_CRITIC_MEMORY at row t equals CRITIC_MEMORY of the window starting at t + 1 wherever t + 1 is a window
 * start, and MEM_OUT at the last row where DONE == 0.
 * PARAMS, critic part: the trunk; W_ih [4 m_v][Hc], W_hh [4 m_v][m_v], b_ih, b_hh [4 m_v]; W_v [m_v], b_v.  Adam, the clip-aware step (one norm
 * over everything), the KL stop, the counters, the normaliser and publish keep their meaning; the critic is never published.
 * Refused with HK_ERR_INVALID, state as it was, the message naming the argument: a NULL r or critic_cell, sequence_length < 1,
 * value_chunk_steps < 0, reserved != 0, a cell whose memory_size is odd or whose m_v is not a multiple of 32 in [32, 128], a NULL weight
 * pointer, a policy without memory and whatever hk_ppo_create_recurrent refuses.  HK_ERR_UNSUPPORTED: hk_ppo_set_precision(HK_PPO_PREC_BF16).
 * Out of scope for recurrent training: a recurrent critic with a feed-forward actor, recurrent POCA, bf16 for either cell or its training
 * products, snapshot pools and self-play swaps of recurrent actors, m_cell above 128, ML-Agents' padding of a trajectory's first, short
 * sequence, burn-in rows.
 * Out of scope (self-play opponent swaps, episode statistics and ELO: "SELF-PLAY" below; POCA and group rewards: "POCA" below):
 * a normaliser for policies attached with normalize == 0,
 * multi-GPU gradient all-reduce and bf16 optimiser state.  Everything is asynchronous on hk_stream unless noted. */
#define HK_PPO_STATS 6
typedef struct hk_ppo_config {
    float gamma;                    /* 0.99 */
    float lambd;                    /* 0.95 */
    int32_t normalize_advantages;   /* 1 */
    float adam_beta1;               /* 0.9 */
    float adam_beta2;               /* 0.999 */
    float adam_eps;                 /* 1e-8 */
    uint32_t seed;                  /* shuffle seed */
} hk_ppo_config;
typedef enum hk_ppo_field {
    HK_PPO_PARAMS = 0, HK_PPO_GRAD, HK_PPO_ADAM_M, HK_PPO_ADAM_V, HK_PPO_V_OLD, HK_PPO_ADV, HK_PPO_RET,
    HK_PPO_MB_MU, HK_PPO_MB_LOGITS, HK_PPO_MB_VALUE, HK_PPO_PERM,
    HK_PPO_SHADOW,      /* uint16 [P + pad]: PARAMS as bf16; the actor's element i at i, the critic's at i + pad, pad = (8 - n_actor % 8) % 8; once
                           the trainer has been in HK_PPO_PREC_BF16 */
    HK_PPO_NORM_MEAN, HK_PPO_NORM_STD,      /* fp32 [in_dim]: the attached policy's published statistics (NORMALISER) */
    HK_PPO_CLIP,        /* fp64 [8]: the result words of the clip-aware step (LONG RUNS); once a clip-aware step has run */
    HK_PPO_FIELDS
} hk_ppo_field;
typedef enum { HK_PPO_PREC_F32 = 0, HK_PPO_PREC_BF16 = 1 } hk_ppo_precision;
int hk_ppo_create(hk_handle h, int policy, const hk_policy_desc* critic, const hk_ppo_config* cfg);
/* the field a recurrent trainer adds (RECURRENT), taken by hk_ppo_ptr / hk_ppo_count beside hk_ppo_field; it lies outside [0, HK_PPO_FIELDS), which is as it was */
typedef enum hk_ppo_recurrent_field {
    HK_PPO_MB_MEMORY = 32      /* fp32 [L][m][2 m_cell]: the memory [h' | c'] each row's cell wrote in the last minibatch; count 0 on other trainers */
} hk_ppo_recurrent_field;
typedef struct hk_ppo_recurrent_desc { int32_t sequence_length, reserved; } hk_ppo_recurrent_desc;
int hk_ppo_create_recurrent(hk_handle h, int policy, const hk_policy_desc* critic, const hk_ppo_config* cfg, const hk_ppo_recurrent_desc* r);
/* the fields a recurrent critic adds (RECURRENT CRITIC); they continue hk_ppo_recurrent_field; count 0 and hk_ppo_ptr refusing on every other trainer */
typedef enum hk_ppo_recurrent_critic_field {
    HK_PPO_CRITIC_MEMORY = 33,       /* fp32 [ceil(R / L)][E][S][2 m_v]: the critic memory carried INTO row k L, before the FIRST rule; after hk_ppo_advantages */
    HK_PPO_CRITIC_MEM_IN = 34,       /* fp32 [E][S][2 m_v]: the critic memory read at row 0 (writable) */
    HK_PPO_CRITIC_MEM_OUT = 35,      /* fp32 [E][S][2 m_v]: the critic memory after row R - 1, zero where DONE[R - 1] (writable) */
    HK_PPO_MB_CRITIC_MEMORY = 36     /* fp32 [L][m][2 m_v]: the memory [h' | c'] each row's critic cell wrote in the last minibatch */
} hk_ppo_recurrent_critic_field;
typedef struct hk_ppo_recurrent_critic_desc {
    int32_t sequence_length;
    int32_t value_chunk_steps;   /* time steps per value-pass launch; 0: the default */
    int32_t reserved[2];         /* 0 */
} hk_ppo_recurrent_critic_desc;
int hk_ppo_create_recurrent_critic(hk_handle h, int policy,
        const hk_policy_desc* critic,            /* trunk; W_mu [m_v], b_mu: the value head */
        const hk_policy_lstm_desc* critic_cell,  /* the critic's own cell */
        const hk_ppo_config* cfg, const hk_ppo_recurrent_critic_desc* r);
int hk_ppo_advantages(hk_handle h, int trainer);
int hk_ppo_minibatch(hk_handle h, int trainer, const int32_t* rows_dev, int m, float eps, float beta, float* stats /*[HK_PPO_STATS]*/);
int hk_ppo_adam(hk_handle h, int trainer, float lr);
int hk_ppo_update(hk_handle h, int trainer, int epochs, int minibatch, float lr, float eps, float beta, float* stats /*[HK_PPO_STATS]*/);
int hk_ppo_publish(hk_handle h, int trainer);
void* hk_ppo_ptr(hk_handle h, int trainer, int field);
int hk_ppo_count(hk_handle h, int trainer, int field);
int hk_ppo_set_precision(hk_handle h, int trainer, int precision);
int hk_ppo_get_precision(hk_handle h, int trainer);
int hk_ppo_gemm_bf16(hk_handle h, int epi, int M, int N, int K, const void* A_dev, const void* B_dev, const float* bias_dev, const float* aux_dev,
                     float* C_dev);
int hk_ppo_normalizer_init(hk_handle h, int trainer, int64_t steps);
int hk_ppo_normalizer_update(hk_handle h, int trainer);
int hk_ppo_normalizer_get(hk_handle h, int trainer, int64_t* steps, double* mean /*[in_dim]*/, double* m2 /*[in_dim]*/);
int hk_ppo_normalizer_set(hk_handle h, int trainer, int64_t steps, const double* mean /*[in_dim]*/, const double* m2 /*[in_dim]*/);
typedef struct hk_ppo_update_opts {
    int32_t epochs, minibatch; float lr, eps, beta;
    float max_grad_norm;   /* 0: off (the plain Adam kernel, no norm); > 0, +inf allowed: clip-aware step; < 0 or NaN: refused */
    float target_kl;       /* 0: off; > 0: stop after an epoch whose mean approx-KL exceeds it; < 0 or NaN: refused */
    int32_t reserved;      /* 0 */
} hk_ppo_update_opts;
typedef struct hk_ppo_update_report {
    int32_t epochs_run, minibatches_run, stopped_by_kl, clipped_steps, nonfinite_steps, reserved;
    double last_epoch_kl, grad_norm_mean, grad_norm_max;    /* the norm figures 0 with clipping off */
} hk_ppo_update_report;
int hk_ppo_update_opt(hk_handle h, int trainer, const hk_ppo_update_opts* o, float* stats /*[HK_PPO_STATS] or NULL*/, hk_ppo_update_report* report /*or NULL*/);
int hk_ppo_adam_clipped(hk_handle h, int trainer, float lr, float max_grad_norm);   /* one clip-aware step from GRAD; max_grad_norm > 0 */
int hk_ppo_get_counters(hk_handle h, int trainer, int64_t* adam_steps, int64_t* epochs_done);
int hk_ppo_set_counters(hk_handle h, int trainer, int64_t adam_steps, int64_t epochs_done);   /* 0 <= each <= INT32_MAX, else refused */

/* ---- POCA: a centralised attention critic, a counterfactual baseline per agent, lambda-returns of the team reward -----------
 * MA-POCA as ML-Agents 2.0 defines it, for the reference's team behaviours (trainer_type: poca).  mlagents was not available to compare
 * against: the rules written here are the contract (as for the ghost trainer's outcome rule in "SELF-PLAY").
 * A POCA trainer is a CRITIC KIND of the trainer table: hk_ppo_create_poca returns a trainer index and every hk_ppo_* entry point takes it.  A
 * trainer made by hk_ppo_create computes what it computed, bit for bit, issues the launches it issued and allocates nothing more.
 * GROUP: the S agent slots of `policy` in one env; 2 <= S <= HK_POCA_MAX_GROUP, all on one team (hk_config.team_of) and every member of it.
 * Every episode end of the reference is EndGroupEpisode, so a group is always complete: there is no attention mask, and ML-Agents' "normalised
 * agent count" input, the constant +1, is dropped (b_val absorbs it) — a documented departure.
 * ROWS, IDS: agent rows as in PPO, id = (t E + e) S + j, n = R E S.  A minibatch id of a POCA trainer is a GROUP id g = t E + e in [0, R E); it
 * stands for the agent rows g S + j.  Under hk_ppo_update / hk_ppo_update_opt `minibatch` counts groups, the permutation is over R E and PERM is
 * int32 [R E].  MB_MU, MB_LOGITS: [m_g S] (x n_branch); MB_VALUE [m_g], one per group; HK_POCA_MB_BASELINE [m_g S].  V_OLD, ADV, RET, HK_POCA_B_OLD,
 * HK_POCA_TEAM_REWARD: [n]; V_OLD holds the group's value once per j.  A group id outside [0, R E) is skipped; stats[5] counts skipped GROUPS.
 * PARAMS / GRAD / ADAM_M / ADAM_V: the actor part exactly as in PPO, then the critic in the order of hk_poca_critic_desc: W_obs, b_obs, W_act,
 * b_act, W_q, b_q, W_k, b_k, W_v, b_v, W_out, b_out, W[0], b[0], ..., w_val, b_val (torch layout, W [out][in]).
 * CRITIC, all fp32.  x_j [in_dim]: the actor's normalised, clipped stacked input of slot j (the actor's normaliser, read in place);
 * a_j = [RAW_j, onehot(BRANCH_j)] [1 + n_branch].
 *   obs entity  uo_j = swish(W_obs x_j + b_obs);   act entity  ua_j = swish(W_act [x_j ; a_j] + b_act)   (one product over the gathered [x ; a])
 *   value sequence (uo_0 ... uo_{S-1});   baseline sequence of agent i: (uo_i, then ua_k for k != i, k ascending)
 *   LN(u) = (u - mean u) / sqrt(var u + 1e-5), population variance over H, no affine
 *   n_s = LN(u_s);  q_s = W_q n_s + b_q;  k_s, v_s alike      (they depend on the entity alone: computed once for a group's 2 S entities)
 *   per head h of HK_POCA_HEADS (width H / 4): score_sr = <q_s^h, k_r^h> / sqrt(H) — the square root of the EMBEDDING size, not the head's (ML-Agents)
 *   alpha_s. = softmax_r(score_sr), the row maximum subtracted;  c_s^h = sum_r alpha_sr v_r^h;  c_s = the four heads side by side
 *   o_s = LN(W_out c_s + b_out + n_s);   z = (1 / S) sum_s o_s     (ML-Agents divides by S + 1e-7: dropped, a documented departure)
 *   y = n_layers x swish(Linear H -> H)(z);   output = <w_val, y> + b_val: ONE head, shared by value and baseline
 *   V(t, e) = the output of the value sequence;   B(t, e, i) = the output of agent i's baseline sequence
 * hk_ppo_advantages on a POCA trainer: V and B over every row, V over the E bootstrap groups, in chunks.  With r, g the transition forms
 * DONE ? TERM_* : * of REWARD and GROUP_REWARD (ML-Agents' lambda_return with add_groupmate_rewards):
 *   rho_{t,e,i} = (sum_k r_{t,e,k}, k ascending, fp32) + g_{t,e,i}                                     -> HK_POCA_TEAM_REWARD
 *   G_{R,i} = V_R (bootstrap);  G_{t,i} = rho_{t,i} + gamma (1 - d_t) [(1 - lambd) V_{t+1} + lambd G_{t+1,i}];  every DONE != 0 terminal
 *   RET = G;  A = G - B;  ADV = normalize_advantages ? (A - mean) / (std + 1e-10) over n (fp64, fixed order) : A;  V_OLD = V, HK_POCA_B_OLD = B
 * LOSS over a minibatch of m = m_g S valid agent rows: L_pi, H, approx-KL and the clip fraction exactly PPO's, on ADV.  Both value losses are
 * PPO's clipped form as means over the m rows, against RET: L_v of v = the row's group value against V_OLD, L_b of b against B_OLD.
 *   L = L_pi + 0.5 (L_v + 0.5 L_b) - beta mean H.       stats[1] stays L_v; L_b comes through hk_poca_stats.
 * In the backward, an entity's gradient is the sum of its sequences' contributions in sequence order.  No float atomics anywhere: the same
 * call on the same state gives the same bits.
 * hk_ppo_adam, hk_ppo_adam_clipped (one norm over actor and POCA critic), hk_ppo_update, hk_ppo_update_opt, hk_ppo_publish, the counters, the
 * normaliser, hk_ppo_ptr / hk_ppo_count and the self-play pool's refusal rule work on a POCA trainer with no further change of meaning.
 * hk_ppo_set_precision(HK_PPO_PREC_BF16) on a POCA trainer: HK_ERR_UNSUPPORTED, the state as it was.
 * hk_ppo_create_poca refuses with HK_ERR_INVALID and a message, nothing allocated: S outside [2, HK_POCA_MAX_GROUP]; slots that are not one
 * whole team; hidden not a multiple of 4 or outside [4, HK_POLICY_MAX_HIDDEN]; n_layers outside [1, HK_POLICY_MAX_LAYERS]; a NULL array;
 * reserved != 0; hk_config.rewards == 0; a bad policy index, a full trainer table or Adam constants out of range (as hk_ppo_create).
 * hk_poca_ptr / hk_poca_count: an HK_POCA_* field of a POCA trainer (another trainer or field is refused).  hk_poca_stats (synchronises):
 * [0] L_b belonging to the stats the last hk_ppo_minibatch / hk_ppo_update(_opt) returned, [1] reserved, 0.
 * Out of scope: bf16 products for the POCA critic, recurrent training (hk_ppo_create_poca refuses a policy with memory), groups that lose members mid-episode (attention masks), a critic normaliser
 * separate from the actor's, multi-GPU gradient all-reduce. */
#define HK_POCA_MAX_GROUP 4
#define HK_POCA_HEADS 4
typedef struct hk_poca_critic_desc {
    int32_t hidden, n_layers, reserved0, reserved1;   /* H % 4 == 0, 4 <= H <= HK_POLICY_MAX_HIDDEN; 1 <= n_layers <= HK_POLICY_MAX_LAYERS */
    const float *W_obs, *b_obs;      /* [H][in_dim], [H]                  obs-only entity embedding           */
    const float *W_act, *b_act;      /* [H][in_dim + 1 + n_branch], [H]   obs+action entity embedding         */
    const float *W_q, *b_q, *W_k, *b_k, *W_v, *b_v, *W_out, *b_out;   /* [H][H], [H] each                     */
    const float *W[HK_POLICY_MAX_LAYERS], *b[HK_POLICY_MAX_LAYERS];   /* encoder, [H][H], [H]                 */
    const float *w_val, *b_val;      /* [H], [1]: ONE head, shared by value and baseline                      */
} hk_poca_critic_desc;
typedef enum hk_poca_field { HK_POCA_B_OLD = 0, HK_POCA_MB_BASELINE, HK_POCA_TEAM_REWARD, HK_POCA_FIELDS } hk_poca_field;
#define HK_POCA_STATS 2              /* [0] L_b, [1] reserved 0 */
int hk_ppo_create_poca(hk_handle h, int policy, const hk_poca_critic_desc* critic, const hk_ppo_config* cfg);
void* hk_poca_ptr(hk_handle h, int trainer, int field);
int hk_poca_count(hk_handle h, int trainer, int field);
int hk_poca_stats(hk_handle h, int trainer, float* out /*[HK_POCA_STATS]*/);   /* synchronises; L_b belonging to the stats the last minibatch / update returned */

/* ---- SELF-PLAY: snapshot pool, opponent swaps, episode statistics of a closed rollout -------------------------------------
 * What ML-Agents' `self_play:` block needs of the library; the driver (window, save_steps / swap_steps, ELO, the linear schedules) is host
 * code: hierarchicalkarting_amd/selfplay.py.  Everything here is opt-in: a handle that never calls these entry points computes what it
 * computed, bit for bit, and allocates nothing.
 * SNAPSHOT POOL.  A pool is `slots` device slots of one SHAPE — in_dim, stack, hidden, n_layers, n_branch and normalize of the policy it was
 * created from.  A slot holds one actor: its flat fp32 parameters in the trainer's torch layout (the actor part of HK_PPO_PARAMS: W[0], b[0],
 * ..., W_mu, b_mu, log_sigma, W_branch, b_branch), followed for a normalize == 1 shape by mean [in_dim] and std [in_dim], the published fp32
 * statistics: hk_policy_pool_count floats.  seed, deterministic, the agent slots, the observation ring and the precision belong to the
 * attached policy and are never touched by a load.
 *   hk_policy_pool_create   -> pool index (up to HK_MAX_POOLS per handle); 1 <= slots <= HK_POOL_MAX_SLOTS
 *   hk_policy_pool_save     the policy's CURRENT fp32 inference copies and published statistics -> slot; asynchronous on hk_stream
 *   hk_policy_pool_load     slot -> the policy's inference copies (the transposed weights, the group-major copy, biases, heads), its mean / std,
 *                           and its bf16 copies if they exist (rebuilt from the fp32 copies just written, as hk_ppo_publish does); asynchronous.
 *                           Every consumer follows: hk_step's decisions, hk_policy_forward, both precisions.
 *   hk_policy_pool_put / _get   a slot from / to a host array of hk_policy_pool_count floats (both synchronise)
 * Refused with HK_ERR_INVALID and a message, state as it was: a bad pool, slot or policy index; a policy whose shape differs from the pool's;
 * a load or get of a slot never written; a load while a rollout is open (the rows of one rollout come from one chain); a load into a policy
 * that has a PPO trainer (its master weights would silently disagree with what plays: train the learner, swap the opponent); a NULL host pointer.
 * RECURRENT POOLS (hk_policy_pool_create_recurrent).  hk_policy_pool_create refuses a policy with memory (HK_ERR_UNSUPPORTED), and so do save and
 * load of such a policy with a pool it made; pools of recurrent actors come from this entry point, which returns an index of the SAME table
 * (HK_MAX_POOLS and HK_POOL_MAX_SLOTS are shared, every hk_policy_pool_* call takes the index).  `policy` must HAVE memory (HK_ERR_INVALID
 * otherwise: use hk_policy_pool_create).  The SHAPE is the feed-forward shape plus the cell's memory_size.  A slot is the actor in the
 * recurrent trainer's torch layout — the actor part of HK_PPO_PARAMS of hk_ppo_create_recurrent: the trunk W[0], b[0], ..., then
 * W_ih [4m][hidden], W_hh [4m][m], b_ih [4m], b_hh [4m] (gates i f g o), then the m-wide heads W_mu [m], b_mu, log_sigma, W_branch [n_branch][m],
 * b_branch — followed by mean and std [in_dim] when the shape normalises.
 *   save   reads the policy's current inference copies: the transposed trunk weights, the group-major Wq_ih / Wq_hh, the RAW b_ih / b_hh that
 *          hk_policy_attach_lstm keeps beside their sum, the heads and the published statistics.  Asynchronous on hk_stream.
 *   load   writes exactly what hk_ppo_publish of a recurrent trainer whose actor parameters equal the slot would write, the summed bias
 *          fp32(b_ih + b_hh) and the raw biases included, then mean / std.  Asynchronous.  The only float operation is that one sum.
 *          It leaves the policy's MEMORY as it was (ML-Agents' ghost swap: load_weights keeps the memories), and as for every load the
 *          observation ring, seed, deterministic, agent slots and decision counters.  hk_policy_memory_clear after it starts the new
 *          weights from a zero memory.
 * Refused with HK_ERR_INVALID as above, and: a policy without memory, of another memory_size, or with another feed-forward shape field.
 * EPISODE STATISTICS (hk_rollout_episode_stats; synchronises) of the COMPLETED rows of the closed rollout, over the agent slots (e, j) of
 * `policy`.  Per (e, j), t ascending, every operation one fp32 operation (no fused multiply-add), so a numpy fp32 loop restates it bit for bit:
 *   acc = carry_ret; gacc = carry_gret; len = carry_len           (0 where there is no valid carry)
 *   row t, DONE == 0:  acc += REWARD; gacc += GROUP_REWARD; len += 1
 *   row t, DONE != 0:  acc += TERM_REWARD; gacc += TERM_GROUP_REWARD; len += 1;  EMIT(acc, gacc, len, DONE, f);
 *                      acc = REWARD; gacc = GROUP_REWARD; len = 0   (the part after the reset belongs to the new episode)
 *   f = TERM_REWARD + TERM_GROUP_REWARD of that row (one fp32 add): f > 0 a win, f < 0 a loss, anything else a draw (+0, -0, an exact
 *   cancellation and a NaN are draws).  DONE == 2 (the time-out) is an episode end like any other and is also tallied in timeouts.
 * This is the outcome rule of ML-Agents 2.0.1's ghost trainer as the maintainers read it (the last step's reward plus group reward; every episode
 * end of the reference is EndGroupEpisode, never an interruption).  mlagents was not available to compare against: the rules written here are the contract.
 * An emitted episode whose beginning lies before the rollout with no valid carry is counted in `partial` and nowhere else.  len_sum is in
 * decisions; ret_* (acc) and gret_* (gacc) are over the emitted, non-partial episodes, summed across episodes in fp64: each lane keeps its own
 * partial record, one workgroup combines the records in (e, j) order — no float atomics, the same call gives the same bits.  ret_min / ret_max
 * are +inf / -inf when episodes == 0.
 * CARRY.  The call is idempotent: it reads a carry-in and writes a carry-out (acc, gacc, len per [E][A], and whether that episode began inside
 * the chain).  hk_rollout_begin adopts the carry-out as the new rollout's carry-in for a policy only if the previous rollout's statistics were
 * computed for that policy and no hk_step, hk_reset, hk_set_agent_state, hk_set_env_state or hk_policy_attach ran between that close and this
 * begin; otherwise the carry is cleared.  The adoption is host code.  A carried episode that began before the first rollout of such a chain
 * stays partial when it ends, in whichever rollout that is.
 * Refused with HK_ERR_INVALID: no closed rollout with a completed row, a rollout open, a bad policy index (or one attached after the rollout
 * began), out == NULL, hk_config.rewards == 0.
 * ELO (host code, selfplay.elo_apply): ML-Agents applies each finished episode's own result in arrival order.  Thousands of episodes end together
 * here and have no order, so a rollout's W wins, D draws and L losses are applied as n = W + D + L sequential steps of the MEAN result
 * s = (W + D / 2) / n: change = k (s - 1 / (1 + 10^((r_opp - r_learner) / 400))), r_learner += change, r_opp -= change.  Order-free, equal to
 * ML-Agents' sequence when all results agree, and self-limiting where a one-shot change of n (s - e) would move ratings by thousands of points.
 * Out of scope: team_change (a trainer is bound to one policy), per-env opponents, bf16 POCA. */
#define HK_MAX_POOLS 8
#define HK_POOL_MAX_SLOTS 64
int hk_policy_pool_create(hk_handle h, int policy, int slots);
int hk_policy_pool_create_recurrent(hk_handle h, int policy, int slots);
int hk_policy_pool_save(hk_handle h, int pool, int slot, int policy);
int hk_policy_pool_load(hk_handle h, int pool, int slot, int policy);
int hk_policy_pool_put(hk_handle h, int pool, int slot, const float* flat /*host [hk_policy_pool_count]*/);
int hk_policy_pool_get(hk_handle h, int pool, int slot, float* flat /*host [hk_policy_pool_count]*/);
int hk_policy_pool_count(hk_handle h, int pool);       /* floats per slot (>= 0), or a negative hk_status */
typedef struct hk_episode_stats {
    int64_t episodes, partial, wins, draws, losses, timeouts, len_sum;
    double ret_sum, ret_sumsq, ret_min, ret_max, gret_sum, gret_sumsq;
} hk_episode_stats;
int hk_rollout_episode_stats(hk_handle h, int policy, hk_episode_stats* out);

/* ---- multi-GPU: the path's ONE exchange step ---------------------------------------------------------------
 * Race instances are independent (one RacingEnvController owns its own Agents[] / Sections[], REC:46-52): every rank steps its
 * own contiguous env-id range (hk_config.env_id_base) and nothing crosses GPUs on the data path.  What a host wants at the end
 * of an episode batch — the reference writes it to ExperimentLogs/ (REC:249-265) — is every race's result: one all-gather of
 * hk_episode_result[E][A] over RCCL (xGMI inside a node).  librccl.so is loaded on the first hk_comm_* call, so single-GPU users
 * do not need it.  Bootstrap as with NCCL: rank 0 obtains an id, the host passes it to every rank by whatever channel it has
 * (MPI, a file, torch.distributed's store, ...), every rank calls hk_comm_init.  One communicator per handle. */
#define HK_COMM_ID_BYTES 128
int hk_comm_unique_id(void* id_out /*[HK_COMM_ID_BYTES]*/);
int hk_comm_init(hk_handle h, int world_size, int rank, const void* id /*[HK_COMM_ID_BYTES]*/);
/* all[E_total][A] (host pointer), the ranks' rows in rank order.  Ranks may hold different env counts (a contiguous split of a
 * total the world size does not divide): the byte counts are exchanged first and the contributions padded on the wire.
 * hk_gather_count returns E_total (the sum of every rank's num_envs) so the caller can size `all`. */
int hk_gather_count(hk_handle h, int64_t* total_envs);
int hk_gather_results(hk_handle h, hk_episode_result* all);
int hk_comm_destroy(hk_handle h);

/* timing taps for bench.py's roofline object: accumulated HIP-event time (ms) and launch count per kernel stage since
 * the last hk_prof_reset.  Stages: [0] env_run_kernel (the fused tick kernel), [1] the lqn_kernel<2,3,4> launches of a
 * round (one bracket), [2] lq_batch_kernel, [3] policy_mlp_kernel,
 * [4] env_observe_kernel + policy_stack_kernel of a decision tick, [5] env_b1_kernel (phase B1 of the solve tick when the tick kernel runs without it).  Events are recorded on the handle's own stream around every launch
 * (no host sync per launch; the tick kernel and the solver launch of a round share the event between them) and folded when read. */
#define HK_PROF_STAGES 6
int hk_prof_enable(hk_handle h, int on);
int hk_prof_reset(hk_handle h);
int hk_prof_read(hk_handle h, double* ms /*[HK_PROF_STAGES]*/, int64_t* launches /*[HK_PROF_STAGES]*/);
/* multi-player LQ games (KartLQR.solveFeedbackLQR calls with N >= 2 players) solved since the last hk_prof_reset, by player count: games[N],
 * N = 2 .. HK_MAX_AGENTS — one per ego per solve tick that holds one, wherever it is solved (a solver launch or in-wave in env_b1_kernel), counted once
 * (single-player games are solved inside the tick / B1 kernel and not counted).  The one rule by which they differ from the reference's solves: the
 * solve ticks of the start hold after its first cadence (cadence < episode step < start_hold_ticks) are skipped — the karts cannot move and each solve
 * would decode the controls of the one before bit for bit — while the skip is on (no planner, no Training-mode reset, HK_NO_HOLD_DEDUPE unset, and no
 * hk_set_agent_state / hk_set_env_state since hk_create).  With that rule the counts equal the CPU oracle's tally (hko_game_counts) for every schedule
 * and call size (tests/test_game_counts_gpu.py).  games[0], games[1] (round 6): the solver passes the waves of env_b1_kernel ran in-wave, and
 * the waves that ran any — their ratio says how well the regroup keeps the envs that hold games apart (1.00: one pass per wave); passes <= in-wave games. */
int hk_prof_games(hk_handle h, int64_t* games /*[HK_MAX_AGENTS + 1]*/);
/* the games-per-launch meter the host picks its schedule from (env_b1_kernel, 4-agent fission handles; hk_prof_games' synchronisation): four words per
 * part p of the batch (0 unsplit; 0 .. 1 on two streams), words[4 p + k]: k = 0 .. 2 the multi-player games (egos that hold one) of the part's B1
 * launches, launch j of the part counting into slot j % 3, and k = 3 the decaying maximum of the finished launches' totals (m <- max(total, m - m / 4)).
 * Read-only; not reset by hk_prof_reset.  The last look at it is hk_schedule_info()'s "games_meter_value". */
#define HK_METER_PARTS 4
int hk_prof_meter(hk_handle h, int64_t* words /*[4 * HK_METER_PARTS]*/);

#ifdef __cplusplus
}
#endif
#endif /* HK_H */
