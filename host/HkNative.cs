// HkNative.cs — P/Invoke binding of libhk.so (include/hk.h, HK_ABI_VERSION 6) for the reference's Unity C# host.
//
// Drop it under Assets/Karting/Scripts/AI/Native/ with libhk.so in Assets/Plugins/x86_64.  Every struct mirrors its C
// twin field for field (tests/test_csharp_layout.py parses this file and checks field order, types, array lengths and
// sizes against the ctypes mirror of hk.h, so the two cannot drift apart unnoticed); every [DllImport] names an exported symbol.
// dotnet / mono / Unity are not part of the build image: this file is source, compiled only where the host lives.
using System;
using System.Runtime.InteropServices;

namespace KartGame.AI.Native
{
    public static class HkConst
    {
        public const int HK_ABI_VERSION = 6;
        public const int HK_MAX_AGENTS = 8;
        public const int HK_MAX_SECTIONS = 64;
        public const int HK_NUM_SENSORS = 9;
        public const int HK_MCTS_MAX_DEPTH = 8;
        public const int HK_MCTS_SECTIME_RING = 8;
        public const int HK_MCTS_MAX_ROOT_PHASES = 3;
        public const int HK_COMM_ID_BYTES = 128;
        public const int HK_PROF_STAGES = 6;
        public const int HK_METER_PARTS = 4;
        public const int HK_MAX_POOLS = 8, HK_POOL_MAX_SLOTS = 64;
        // hk_rollout_field: the buffers of the rollout recorder (hk_rollout_ptr)
        public const int HK_RO_OBS = 0, HK_RO_FIRST = 1, HK_RO_STEER = 2, HK_RO_BRANCH = 3, HK_RO_RAW = 4, HK_RO_MU = 5, HK_RO_LOGITS = 6,
                         HK_RO_LOGP_CONT = 7, HK_RO_LOGP_DISC = 8, HK_RO_REWARD = 9, HK_RO_GROUP_REWARD = 10, HK_RO_TERM_REWARD = 11,
                         HK_RO_TERM_GROUP_REWARD = 12, HK_RO_DONE = 13, HK_RO_RING0 = 14, HK_RO_NEXT_OBS = 15, HK_RO_MEMORY = 16,
                         HK_RO_NEXT_MEMORY = 17, HK_RO_FIELDS = 18;      // MEMORY / NEXT_MEMORY: recurrent actors only (NULL pointer otherwise)
        public const int HK_POLICY_MAX_MEMORY = 256;
        // hk_ppo_field: the PPO trainer's buffers (hk_ppo_ptr / hk_ppo_count); HK_PPO_STATS: L_pi, L_v, entropy, approx-KL, clip fraction, skipped rows
        public const int HK_PPO_PARAMS = 0, HK_PPO_GRAD = 1, HK_PPO_ADAM_M = 2, HK_PPO_ADAM_V = 3, HK_PPO_V_OLD = 4, HK_PPO_ADV = 5, HK_PPO_RET = 6,
                         HK_PPO_MB_MU = 7, HK_PPO_MB_LOGITS = 8, HK_PPO_MB_VALUE = 9, HK_PPO_PERM = 10, HK_PPO_SHADOW = 11, HK_PPO_NORM_MEAN = 12, HK_PPO_NORM_STD = 13, HK_PPO_CLIP = 14, HK_PPO_FIELDS = 15,
                         HK_PPO_PREC_F32 = 0, HK_PPO_PREC_BF16 = 1,
                         HK_POLICY_PREC_F32 = 0, HK_POLICY_PREC_BF16 = 1,      // hk_policy_precision
                         HK_PPO_STATS = 6;
        public const int HK_PPO_MB_MEMORY = 32;      // hk_ppo_recurrent_field: a recurrent trainer's extra buffer, outside [0, HK_PPO_FIELDS)
        public const int HK_PPO_CRITIC_MEMORY = 33, HK_PPO_CRITIC_MEM_IN = 34, HK_PPO_CRITIC_MEM_OUT = 35, HK_PPO_MB_CRITIC_MEMORY = 36;      // hk_ppo_recurrent_critic_field
        // hk_poca_field: the extra buffers of a POCA trainer (hk_poca_ptr / hk_poca_count); HK_POCA_STATS: L_b, reserved
        public const int HK_POCA_B_OLD = 0, HK_POCA_MB_BASELINE = 1, HK_POCA_TEAM_REWARD = 2, HK_POCA_FIELDS = 3, HK_POCA_STATS = 2,
                         HK_POCA_MAX_GROUP = 4, HK_POCA_HEADS = 4;
        // HierarchicalKartAgent.cs:21-33
        public const int HK_LOW_RL = 0, HK_LOW_MPC = 1, HK_LOW_LQR = 2, HK_LOW_E2E = 3;   // E2E: EndToEndKartAgent
        public const int HK_HIGH_MCTS = 0, HK_HIGH_FIXED = 1, HK_HIGH_NONE = 2;   // NONE: E2E with runQuasiMCTS off
        // RacingEnvController.cs:24-29
        public const int HK_MODE_RACE = 0, HK_MODE_TRAINING = 1, HK_MODE_EXPERIMENT = 2;
        // hk_agent_state.flags
        public const uint HK_F_ACCEL = 1u << 0, HK_F_BRAKE = 1u << 1, HK_F_ACTIVE = 1u << 2, HK_F_FORWARD_COLLISION = 1u << 3,
                          HK_F_HAS_COLLISION = 1u << 4, HK_F_CAN_MOVE = 1u << 5, HK_F_ENABLED = 1u << 6;
    }

    // hk_kart_stats: ArcadeKart.Stats (KartSystems/ArcadeKart.cs:20-69)
    [StructLayout(LayoutKind.Sequential)]
    public struct HkKartStats
    {
        public float TopSpeed;
        public float Acceleration;
        public float ReverseSpeed;
        public float ReverseAcceleration;
        public float AccelerationCurve;
        public float Braking;
        public float CoastingDrag;
        public float Grip;
        public float MaxSteer;
        public float MinSteer;
        public float TireWearFactor;
        public float MinGs;
        public float MaxGs;
        public float AddedGravity;
        public float TireWearRate;
        public float AngularDrag;
    }

    // hk_section: one DiscretePositionTracker (DiscretePositionTracker.cs:20-44) with its Waypoint prefab geometry
    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct HkSection
    {
        public float trig_x;
        public float trig_z;
        public float yaw_deg;
        public float marker_y;
        public fixed float lane_x[4];
        public fixed float lane_z[4];
        public float track_inside_radius;
        public float track_length;
        public float track_width;
        public float turn_degrees;
        public int left_turn;
        public int optimal_lane;
    }

    // hk_wall_seg
    [StructLayout(LayoutKind.Sequential)]
    public struct HkWallSeg
    {
        public float x0;
        public float z0;
        public float x1;
        public float z1;
    }

    // hk_reward_params: RacingEnvController reward fields (REC:65-108)
    [StructLayout(LayoutKind.Sequential)]
    public struct HkRewardParams
    {
        public float WallHitPenalty;
        public float OpponentHitPenalty;
        public float HitByOpponentPenalty;
        public float PassCheckpointLaneReward;
        public float PassCheckpointVelocityReward;
        public float PassCheckpointBase;
        public float PassCheckpointTimeMultiplier;
        public float TeamPassCheckpointBase;
        public float TeamPassCheckpointTimeMultiplier;
        public float BeingBehindOpponentCheckpointPenalty;
        public float BeingBehindTeammateCheckpointPenalty;
        public float TeamScoreRewardMultiplier;
        public float ReversePenalty;
        public float SwervingPenalty;
        public float ReachGoalCheckpointRewardMultplier;
        public float ReachGoalCheckpointRewardBase;
        public float TowardsCheckpointReward;
        public float SpeedReward;
        public float SlowMovingPenalty;
        public float AccelerationReward;
        public float NotAtGoalPenalty;
    }

    // hk_engine_params: the engine restatement's constants (Rigidbody / CapsuleCollider / WheelCollider / KartAnimation values of the kart prefab)
    [StructLayout(LayoutKind.Sequential)]
    public struct HkEngineParams
    {
        public float mass;
        public float inertia_y;
        public float gravity;
        public float axle_zf;
        public float axle_zr;
        public float max_steer_deg;
        public float steer_damping;
        public float side_ext_slip;
        public float side_ext_value;
        public float side_asy_slip;
        public float side_asy_value;
        public float side_stiffness;
        public float side_slope0;
        public float slip_min_speed;
        public float wheel_mass;
        public float wheel_radius_f;
        public float wheel_radius_r;
        public float wheel_damping;
        public float fwd_ext_slip;
        public float fwd_ext_value;
        public float fwd_asy_slip;
        public float fwd_asy_value;
        public float fwd_stiffness;
        public float long_slip_min_speed;
        public int wheel_friction;
        public int contact_yaw;
        public int wheel_rolling;
    }

    // hk_config
    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct HkConfig
    {
        public int abi_version;
        public int num_envs;
        public int num_agents;
        public int device_id;
        public fixed int team_of[8];
        public fixed int n_team[8];
        public fixed int team_agents[64];
        public fixed int n_other[8];
        public fixed int other_agents[64];
        public fixed int high_mode[8];
        public fixed int low_mode[8];
        public fixed int tree_search_depth[8];
        public fixed int velocity_bucket_size[8];
        public HkKartStats stats;
        public int laps;
        public int max_episode_steps;
        public int max_lane_changes;
        public int section_horizon;
        public int disable_on_end;
        public int env_mode;
        public int start_hold_ticks;
        public int auto_reset;
        public float dt;
        public float kart_y;
        public fixed float sensor_yaw_deg[9];
        public fixed float ray_distance[9];
        public fixed float wall_hit_validation[9];
        public fixed float agent_hit_validation[9];
        public uint jitter_seed;
        public float jitter_pos;
        public float jitter_yaw;
        public int env_id_base;
        public int num_sections;
        public int num_walls;
        public HkSection* sections;
        public HkWallSeg* walls;
        public fixed int time_precision[8];
        public fixed int section_window[8];
        public int mcts_iterations;
        public int mcts_initial_iterations;
        public int mcts_latency_ticks;
        public int mcts_initial_latency_ticks;
        public uint mcts_seed;
        public int rewards;
        public fixed int training_agent[8];
        public HkRewardParams rw;
        public uint train_seed;
        public int debug_taps;
        public HkEngineParams engine;
    }

    // hk_mcts_plan: bestStates (HKA:70,252)
    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct HkMctsPlan
    {
        public int n_states;
        public int n_players;
        public fixed int section[8];
        public fixed byte player_agent[8];
        public fixed byte lane[64];
        public fixed byte vel[64];
    }

    // hk_mcts_state
    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct HkMctsState
    {
        public fixed int sec_time[8];
        public int ready_step;
        public int searches;
        public int root_live;
        public int root_cycles;
        public int pend_kind;
        public int root_phases;
        public HkMctsPlan best;
        public HkMctsPlan pend;
        public fixed byte belief_lane[512];
        public fixed byte belief_vel[512];
    }

    // hk_agent_state: the fields of KartAgent (KA:102-128), ArcadeKart (AK:190-205) and the Rigidbody that survive a tick
    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct HkAgentState
    {
        public float px;
        public float pz;
        public float yaw;
        public float vx;
        public float vz;
        public float wy;
        public float acc_ang_v;
        public float steering;
        public float avg_lane_diff;
        public float avg_vel_diff;
        public float cum_reward;
        public float contact_nx;
        public float contact_nz;
        public int section_index;
        public int lane;
        public int lane_changes;
        public int illegal_lane_changes;
        public int forward_collisions;
        public int last_collision_time;
        public int time_steps;
        public int init_checkpoint_index;
        public uint flags;
        public uint trig_lo;
        public uint trig_hi;
        public float final_steer;
        public int tele_completed_laps;
        public int tele_lap_end_step;
        public float tele_last_lap;
        public float tele_best_lap;
        public float tele_total_time;
        public fixed byte plan_lane[64];
        public fixed float plan_vel[64];
        public float step_reward;
        public float group_reward;
        public float steer_smoothed;
        public float wheel_uf;
        public float wheel_ur;
    }

    // hk_env_state
    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct HkEnvState
    {
        public int episode_steps;
        public uint inactive_mask;
        public int experiment_num;
        public int episodes_done;
        public uint status;
        public int initial_started;
        public fixed int reserved[2];
    }

    // hk_episode_result: TelemetryViewer / experiment-log quantities (TelemetryViewer.cs:49-108)
    [StructLayout(LayoutKind.Sequential)]
    public struct HkEpisodeResult
    {
        public int time_steps;
        public int section_index;
        public int illegal_lane_changes;
        public int forward_collisions;
        public float avg_lane_diff;
        public float avg_vel_diff;
        public float reward;
        public int episode;
        public float last_lap;
        public float best_lap;
        public float total_time;
        public int laps_completed;
        public int lap_end_step;
        public float speed;
        public int active;
        public float group_reward;
    }

    // hk_lq_debug
    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct HkLqDebug
    {
        public int n_players;
        public fixed int player_agent[8];
        public fixed int branch[8];
        public fixed double initial[32];
        public fixed double target[32];
        public fixed double target_w[32];
        public fixed double control_w[8];
        public fixed double u0[2];
    }

    // hk_policy_desc: the ML-Agents actor read from a BehaviorParameters.Model asset (NNModel -> ONNX initialisers)
    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct HkPolicyDesc
    {
        public int in_dim;
        public int stack;
        public int hidden;
        public int n_layers;
        public int n_branch;
        public int normalize;
        public int deterministic;
        public uint seed;
        public float* norm_mean;
        public float* norm_std;
        public float* W0;
        public float* W1;
        public float* W2;
        public float* W3;
        public float* b0;
        public float* b1;
        public float* b2;
        public float* b3;
        public float* W_mu;
        public float* b_mu;
        public float* log_sigma;
        public float* W_branch;
        public float* b_branch;
    }

    // hk_policy_lstm_desc: the LSTM cell of a recurrent actor (NetworkSettings.memory; torch layout, gates i f g o; m = memory_size / 2)
    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct HkPolicyLstmDesc
    {
        public int memory_size;
        public int reserved;
        public float* W_ih;       // [4m][hidden]
        public float* W_hh;       // [4m][m]
        public float* b_ih;       // [4m]
        public float* b_hh;       // [4m]
    }

    // hk_ppo_config: the trainer's constants (ML-Agents trainer_config: gamma, lambd; torch's Adam defaults)
    [StructLayout(LayoutKind.Sequential)]
    public struct HkPpoConfig
    {
        public float gamma;
        public float lambd;
        public int normalize_advantages;
        public float adam_beta1;
        public float adam_beta2;
        public float adam_eps;
        public uint seed;
    }

    // hk_poca_critic_desc: the initial weights of a POCA trainer's attention critic (hk.h "POCA"); torch layout, W [out][in]
    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct HkPocaCriticDesc
    {
        public int hidden;
        public int n_layers;
        public int reserved0;
        public int reserved1;
        public float* W_obs;
        public float* b_obs;
        public float* W_act;
        public float* b_act;
        public float* W_q;
        public float* b_q;
        public float* W_k;
        public float* b_k;
        public float* W_v;
        public float* b_v;
        public float* W_out;
        public float* b_out;
        public float* W0;
        public float* W1;
        public float* W2;
        public float* W3;
        public float* b0;
        public float* b1;
        public float* b2;
        public float* b3;
        public float* w_val;
        public float* b_val;
    }

    // hk_ppo_recurrent_desc: hk_ppo_create_recurrent's sequence length (hk.h "PPO trainer" RECURRENT)
    [StructLayout(LayoutKind.Sequential)]
    public struct HkPpoRecurrentDesc
    {
        public int sequence_length;
        public int reserved;
    }

    // hk_ppo_recurrent_critic_desc: hk_ppo_create_recurrent_critic's sequence length and value-pass chunk (hk.h "PPO trainer" RECURRENT CRITIC)
    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct HkPpoRecurrentCriticDesc
    {
        public int sequence_length;
        public int value_chunk_steps;
        public fixed int reserved[2];
    }

    // hk_ppo_update_opts / hk_ppo_update_report: hk_ppo_update_opt's options (0: off) and what it did (hk.h "LONG RUNS")
    [StructLayout(LayoutKind.Sequential)]
    public struct HkPpoUpdateOpts
    {
        public int epochs;
        public int minibatch;
        public float lr;
        public float eps;
        public float beta;
        public float max_grad_norm;
        public float target_kl;
        public int reserved;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct HkPpoUpdateReport
    {
        public int epochs_run;
        public int minibatches_run;
        public int stopped_by_kl;
        public int clipped_steps;
        public int nonfinite_steps;
        public int reserved;
        public double last_epoch_kl;
        public double grad_norm_mean;
        public double grad_norm_max;
    }

    // hk_episode_stats: returns, lengths and outcomes of the closed rollout's episodes (hk.h "SELF-PLAY")
    [StructLayout(LayoutKind.Sequential)]
    public struct HkEpisodeStats
    {
        public long episodes;
        public long partial;
        public long wins;
        public long draws;
        public long losses;
        public long timeouts;
        public long len_sum;
        public double ret_sum;
        public double ret_sumsq;
        public double ret_min;
        public double ret_max;
        public double gret_sum;
        public double gret_sumsq;
    }

    public static unsafe class Hk
    {
        const string Lib = "hk";   // libhk.so next to the player binary / in Assets/Plugins/x86_64

        // scene instantiation of RacingEnvController + KartAgents (REC.Start :148-168, HKA.Awake :413-426)
        [DllImport(Lib)] public static extern int hk_create(HkConfig* cfg, out IntPtr handle);
        [DllImport(Lib)] public static extern void hk_destroy(IntPtr h);
        [DllImport(Lib)] public static extern IntPtr hk_last_error(IntPtr h);
        // RacingEnvController.ResetGame (REC:499-719)
        [DllImport(Lib)] public static extern int hk_reset(IntPtr h, int* envIds, int n, int experimentNum);
        // KartAgent.OnActionReceived / InterpretDiscreteActions (KA:440-478, HKA:1371-1379)
        [DllImport(Lib)] public static extern int hk_set_actions(IntPtr h, float* steer, int* branch);
        // n Unity FixedUpdate ticks
        [DllImport(Lib)] public static extern int hk_step(IntPtr h, int nTicks);
        // HierarchicalKartAgent.CollectObservations (HKA:485-604)
        [DllImport(Lib)] public static extern int hk_obs_dim(IntPtr h);
        [DllImport(Lib)] public static extern int hk_get_observations(IntPtr h, float* obs);
        [DllImport(Lib)] public static extern int hk_get_agent_state(IntPtr h, HkAgentState* outState);
        [DllImport(Lib)] public static extern int hk_set_agent_state(IntPtr h, HkAgentState* inState);
        [DllImport(Lib)] public static extern int hk_get_env_state(IntPtr h, HkEnvState* outState);
        [DllImport(Lib)] public static extern int hk_set_env_state(IntPtr h, HkEnvState* inState);
        [DllImport(Lib)] public static extern int hk_get_episode_results(IntPtr h, HkEpisodeResult* outRes);
        // Agent.SendInfo: m_Reward / m_GroupReward since the last call (read and reset)
        [DllImport(Lib)] public static extern int hk_get_rewards(IntPtr h, float* reward, float* groupReward);
        [DllImport(Lib)] public static extern int hk_get_lq_debug(IntPtr h, int env, int ego, HkLqDebug* outDbg);
        [DllImport(Lib)] public static extern int hk_get_mcts_state(IntPtr h, HkMctsState* outStates);
        // KartLQR.solveFeedbackLQR (AI/LQR/KartLQR.cs:17), batched
        [DllImport(Lib)] public static extern int hk_lq_solve_batch(IntPtr h, int batch, int N, double* A, double* B, double* Q, double* q,
                                                                  double* R, double* x0, int horizon, double* u0);
        [DllImport(Lib)] public static extern int hk_lq_solve_batch_device(IntPtr h, int batch, int N, IntPtr dA, IntPtr dB, IntPtr dQ, IntPtr dq,
                                                                         IntPtr dR, IntPtr dx0, int horizon, IntPtr du0, IntPtr stream);
        // device-resident surface (an external trainer that keeps its tensors on the GPU)
        [DllImport(Lib)] public static extern IntPtr hk_device_results_ptr(IntPtr h);
        [DllImport(Lib)] public static extern IntPtr hk_device_agents_ptr(IntPtr h);
        [DllImport(Lib)] public static extern int hk_observe(IntPtr h);
        [DllImport(Lib)] public static extern int hk_rewards_device(IntPtr h);
        [DllImport(Lib)] public static extern IntPtr hk_device_obs_ptr(IntPtr h);
        [DllImport(Lib)] public static extern IntPtr hk_device_reward_ptr(IntPtr h);
        [DllImport(Lib)] public static extern IntPtr hk_device_group_reward_ptr(IntPtr h);
        [DllImport(Lib)] public static extern IntPtr hk_device_act_steer_ptr(IntPtr h);
        [DllImport(Lib)] public static extern IntPtr hk_device_act_branch_ptr(IntPtr h);
        [DllImport(Lib)] public static extern IntPtr hk_stream(IntPtr h);
        [DllImport(Lib)] public static extern int hk_synchronize(IntPtr h);
        [DllImport(Lib)] public static extern IntPtr hk_build_info();               // const char* (JSON), owned by the library: Marshal.PtrToStringAnsi
        [DllImport(Lib)] public static extern IntPtr hk_schedule_info(IntPtr h);     // const char* (JSON), owned by the handle
        // LowMode == RL: the actor runs on device every DecisionPeriod ticks instead of Barracuda (KA:440, HKA:1371-1379)
        [DllImport(Lib)] public static extern int hk_policy_attach(IntPtr h, HkPolicyDesc* desc, int* agentSlots, int nSlots, int decisionPeriod);
        [DllImport(Lib)] public static extern int hk_policy_set_precision(IntPtr h, int policy, int precision);
        [DllImport(Lib)] public static extern int hk_policy_get_precision(IntPtr h, int policy);
        [DllImport(Lib)] public static extern int hk_policy_forward(IntPtr h, int policy, int rows, float* obs, float* mu, float* logits);
        // recurrent actors (hk.h "RECURRENT ACTORS"): memory [h | c] of 2m floats per (env, agent slot); lstm == null is hk_policy_attach
        [DllImport(Lib)] public static extern int hk_policy_attach_lstm(IntPtr h, HkPolicyDesc* desc, HkPolicyLstmDesc* lstm, int* agentSlots, int nSlots, int decisionPeriod);
        [DllImport(Lib)] public static extern int hk_policy_memory_size(IntPtr h, int policy);
        [DllImport(Lib)] public static extern int hk_policy_forward_mem(IntPtr h, int policy, int rows, float* obs, float* memIn, float* mu, float* logits, float* memOut);
        [DllImport(Lib)] public static extern int hk_policy_memory_get(IntPtr h, int policy, float* mem);
        [DllImport(Lib)] public static extern int hk_policy_memory_set(IntPtr h, int policy, float* mem);
        [DllImport(Lib)] public static extern int hk_policy_memory_clear(IntPtr h, int policy);
        // recurrent actors in bf16 (hk.h "RECURRENT ACTORS IN BF16"): the policy's switch, the recurrent trainer's, and the gate-product tap on device pointers
        [DllImport(Lib)] public static extern int hk_policy_lstm_set_precision(IntPtr h, int policy, int precision);
        [DllImport(Lib)] public static extern int hk_ppo_recurrent_set_precision(IntPtr h, int trainer, int precision);
        [DllImport(Lib)] public static extern int hk_ppo_lstm_gates_bf16(IntPtr h, int rows, int H, int m, IntPtr aDev, IntPtr hDev, IntPtr wIhDev, IntPtr wHhDev, float* bsumDev, float* zDev);
        [DllImport(Lib)] public static extern int hk_get_actions(IntPtr h, float* steer, int* branch);
        // rollout recorder: every decision of the attached actors writes a row of device buffers (fields: hk.h hk_rollout_field)
        [DllImport(Lib)] public static extern int hk_rollout_begin(IntPtr h, int rows);
        [DllImport(Lib)] public static extern int hk_rollout_rows(IntPtr h);
        [DllImport(Lib)] public static extern int hk_rollout_close(IntPtr h);
        [DllImport(Lib)] public static extern IntPtr hk_rollout_ptr(IntPtr h, int field);
        // PPO trainer: train an attached actor on the closed rollout, on the device (hk.h "PPO trainer")
        [DllImport(Lib)] public static extern int hk_ppo_create(IntPtr h, int policy, HkPolicyDesc* critic, HkPpoConfig* cfg);
        [DllImport(Lib)] public static extern int hk_ppo_create_recurrent(IntPtr h, int policy, HkPolicyDesc* critic, HkPpoConfig* cfg, HkPpoRecurrentDesc* r);
        [DllImport(Lib)] public static extern int hk_ppo_create_recurrent_critic(IntPtr h, int policy, HkPolicyDesc* critic, HkPolicyLstmDesc* criticCell, HkPpoConfig* cfg, HkPpoRecurrentCriticDesc* r);
        [DllImport(Lib)] public static extern int hk_ppo_advantages(IntPtr h, int trainer);
        [DllImport(Lib)] public static extern int hk_ppo_minibatch(IntPtr h, int trainer, IntPtr rowsDev, int m, float eps, float beta, float* stats);
        [DllImport(Lib)] public static extern int hk_ppo_adam(IntPtr h, int trainer, float lr);
        [DllImport(Lib)] public static extern int hk_ppo_update(IntPtr h, int trainer, int epochs, int minibatch, float lr, float eps, float beta, float* stats);
        [DllImport(Lib)] public static extern int hk_ppo_publish(IntPtr h, int trainer);
        [DllImport(Lib)] public static extern IntPtr hk_ppo_ptr(IntPtr h, int trainer, int field);
        [DllImport(Lib)] public static extern int hk_ppo_count(IntPtr h, int trainer, int field);
        [DllImport(Lib)] public static extern int hk_ppo_set_precision(IntPtr h, int trainer, int precision);
        [DllImport(Lib)] public static extern int hk_ppo_get_precision(IntPtr h, int trainer);
        [DllImport(Lib)] public static extern int hk_ppo_gemm_bf16(IntPtr h, int epi, int M, int N, int K, IntPtr aDev, IntPtr bDev, float* biasDev, float* auxDev, float* cDev);
        // the running normaliser of a trainer's actor (hk.h "PPO trainer" NORMALISER): fp64 state per trainer, published into the attached policy
        [DllImport(Lib)] public static extern int hk_ppo_normalizer_init(IntPtr h, int trainer, long steps);
        [DllImport(Lib)] public static extern int hk_ppo_normalizer_update(IntPtr h, int trainer);
        [DllImport(Lib)] public static extern int hk_ppo_normalizer_get(IntPtr h, int trainer, long* steps, double* mean, double* m2);
        [DllImport(Lib)] public static extern int hk_ppo_normalizer_set(IntPtr h, int trainer, long steps, double* mean, double* m2);
        // long runs: clip by the global norm, KL stop, and the two counters a resumed trainer needs
        [DllImport(Lib)] public static extern int hk_ppo_update_opt(IntPtr h, int trainer, HkPpoUpdateOpts* o, float* stats, HkPpoUpdateReport* report);
        [DllImport(Lib)] public static extern int hk_ppo_adam_clipped(IntPtr h, int trainer, float lr, float maxGradNorm);
        [DllImport(Lib)] public static extern int hk_ppo_get_counters(IntPtr h, int trainer, long* adamSteps, long* epochsDone);
        [DllImport(Lib)] public static extern int hk_ppo_set_counters(IntPtr h, int trainer, long adamSteps, long epochsDone);
        // POCA (hk.h "POCA"): a trainer whose critic is the team's attention critic; every hk_ppo_* entry point takes its index
        [DllImport(Lib)] public static extern int hk_ppo_create_poca(IntPtr h, int policy, HkPocaCriticDesc* critic, HkPpoConfig* cfg);
        [DllImport(Lib)] public static extern IntPtr hk_poca_ptr(IntPtr h, int trainer, int field);
        [DllImport(Lib)] public static extern int hk_poca_count(IntPtr h, int trainer, int field);
        [DllImport(Lib)] public static extern int hk_poca_stats(IntPtr h, int trainer, float* stats);
        // self-play (hk.h "SELF-PLAY"): device slots of saved actors, loaded into an attached opponent; episode statistics of the closed rollout
        [DllImport(Lib)] public static extern int hk_policy_pool_create(IntPtr h, int policy, int slots);
        // a pool of recurrent actors (the policy must have memory): an index of the same table, a slot in the recurrent trainer's layout
        [DllImport(Lib)] public static extern int hk_policy_pool_create_recurrent(IntPtr h, int policy, int slots);
        [DllImport(Lib)] public static extern int hk_policy_pool_save(IntPtr h, int pool, int slot, int policy);
        [DllImport(Lib)] public static extern int hk_policy_pool_load(IntPtr h, int pool, int slot, int policy);
        [DllImport(Lib)] public static extern int hk_policy_pool_put(IntPtr h, int pool, int slot, float* flat);
        [DllImport(Lib)] public static extern int hk_policy_pool_get(IntPtr h, int pool, int slot, float* flat);
        [DllImport(Lib)] public static extern int hk_policy_pool_count(IntPtr h, int pool);
        [DllImport(Lib)] public static extern int hk_rollout_episode_stats(IntPtr h, int policy, HkEpisodeStats* stats);
        // multi-GPU: one process per GPU, envs sharded by HkConfig.env_id_base; the only exchange is this all-gather over RCCL
        [DllImport(Lib)] public static extern int hk_comm_unique_id(byte* id128);
        [DllImport(Lib)] public static extern int hk_comm_init(IntPtr h, int worldSize, int rank, byte* id128);
        [DllImport(Lib)] public static extern int hk_gather_count(IntPtr h, long* totalEnvs);
        [DllImport(Lib)] public static extern int hk_gather_results(IntPtr h, HkEpisodeResult* all);
        [DllImport(Lib)] public static extern int hk_comm_destroy(IntPtr h);
        // timing taps
        [DllImport(Lib)] public static extern int hk_prof_enable(IntPtr h, int on);
        [DllImport(Lib)] public static extern int hk_prof_reset(IntPtr h);
        [DllImport(Lib)] public static extern int hk_prof_read(IntPtr h, double* ms, long* launches);
        [DllImport(Lib)] public static extern int hk_prof_games(IntPtr h, long* games);
        [DllImport(Lib)] public static extern int hk_prof_meter(IntPtr h, long* words);     // [4 * HK_METER_PARTS]

        public static void Check(int rc, IntPtr h)
        {
            if (rc < 0) throw new InvalidOperationException("libhk error " + rc + ": " + Marshal.PtrToStringAnsi(hk_last_error(h)));
        }
    }
}
