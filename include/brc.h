/*
 * brc.h -- C-ABI of the MI355X batched consensus engine (libbrc_hip.so).
 *
 * Drop-in boundary for the reference's hot path.  The reference exposes it as Python
 * classes; this ABI is what those classes (re-implemented in
 * byzantinerandomizedconsensus_amd/) bind through ctypes:
 *
 *   reference                                                   replaced by
 *   ---------------------------------------------------------   ----------------------------
 *   BRBroadcast.__init__ / ByzantineRandomizedConsensus.__init__ brc_create
 *     (core/brbroadcast.py:17-44, core/byzantinerandomizedconsensus.py:18-36)
 *   BRBroadcast.broadcast_listener (core/brbroadcast.py:121-128) brc_run (the accept loop,
 *     + the listener loop body (core/brbroadcast.py:60-119)       batched over instances)
 *   Broadcast.broadcast(SEND, m)     (base/broadcast.py:17-40)   brc_inject(BRC_INJ_SEND)
 *   ByzantineRandomizedConsensus.start/propose (:38-51)          brc_inject(BRC_INJ_PROPOSE) /
 *                                                                brc_load_proposals
 *   IBroadcastHandler.deliver upcall (base/broadcast.py:52-55)   brc_read_events (DELIVER)
 *   IConsensusHandler.decide upcall  (base/consensus.py:22-24)   brc_read_events (DECIDE),
 *                                                                brc_read_replicas
 *   (Byzantine peers: raw sends into the transport)              brc_inject(BRC_INJ_KEY/SEND/MSG),
 *                                                                brc_load_byzantine
 *
 * Conventions: every call returns 0 on success or a negative BRC_E_* code; host buffers
 * are caller-owned; device buffers are engine-owned; one host thread per engine; all work
 * is ordered on the engine's own HIP stream; no callbacks cross the ABI.
 */
#ifndef BRC_H
#define BRC_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BRC_ABI_VERSION 13

enum {
    BRC_OK = 0,
    BRC_E_INVALID = -1,      /* bad argument / unsupported configuration */
    BRC_E_NOMEM = -2,        /* device or host allocation failed */
    BRC_E_HIP = -3,          /* HIP runtime error (see brc_last_error) */
    BRC_E_UNSUPPORTED = -4,  /* a workload feature the engine does not model */
    BRC_E_STATE = -5         /* call not valid in the current engine state */
};

enum { BRC_PROTO_BRB = 0, BRC_PROTO_CONSENSUS = 1 };
/* BRC_MODE_REFERENCE: the protocol exactly as the reference runs it, quirks included (SURVEY §4
 * K1-K12).  BRC_MODE_SPEC: the protocol the reference intends (Bracha-correct broadcast; consensus
 * with per-phase windows and the core/byzantinerandomizedconsensus.py:88-92 coin made reachable as
 * a common Philox coin keyed (coin_seed, instance, round)). */
/* BRC_MODE_BEB: best-effort broadcast (core/bebroadcast.py as intended -- the reference's class
 * cannot be constructed): a SEND delivers at its arrival, no ECHO/READY; with BRC_PROTO_CONSENSUS
 * the reference's consensus runs on top of it (its consensus_instance.deliver, :42). */
enum { BRC_MODE_REFERENCE = 0, BRC_MODE_SPEC = 1, BRC_MODE_BEB = 2 };
/* Peer identity of core/brbroadcast.py:69-71.  SENDER (:71): sets hold sender ids and the
 * network drops a message identical to one already sent on the link.  CONNECTION (:69, the
 * reference's local-test mode): every message is its own connection -- a new peer -- so sets
 * count messages, nothing is dropped, and the :119 amplification re-fires on every qualifying READY.
 * CONNECTION needs BRC_MODE_REFERENCE (any n <= 256, delay_max <= 16); it keeps per-cell send
 * counts of one byte, so an injection of a 256th copy of one type by one replica in one step stops
 * the instance with BRC_BADINJ. */
enum { BRC_PEER_SENDER = 0, BRC_PEER_CONNECTION = 1 };
enum { BRC_DELAY_CONST = 0, BRC_DELAY_UNIFORM = 1, BRC_DELAY_SLOWSET = 2, BRC_DELAY_GEOMETRIC = 3 };
enum { BRC_PROPOSALS_NONE = 0, BRC_PROPOSALS_PHILOX = 1, BRC_PROPOSALS_LOADED = 2 };
enum { BRC_BYZ_NONE = 0, BRC_BYZ_EQUIVOCATE = 1 };
enum { BRC_SEND = 1, BRC_ECHO = 2, BRC_READY = 3 };
/* BRC_INJ_DELIVER: ByzantineRandomizedConsensus.deliver(message) called directly on replica `node`
 * (core/byzantinerandomizedconsensus.py:53) with a message of host `kp` (a replica id) carrying
 * value id `value` -- no BRB traffic; the consensus logic runs as on a BRB delivery.  Consensus
 * protocol, BRC_MODE_REFERENCE or BRC_MODE_BEB (BRC_MODE_SPEC counts phases: BRC_E_UNSUPPORTED). */
enum { BRC_INJ_PROPOSE = 1, BRC_INJ_SEND = 2, BRC_INJ_KEY = 3, BRC_INJ_MSG = 4, BRC_INJ_DELIVER = 5 };
enum { BRC_RUNNING = 0, BRC_DONE = 1, BRC_QUIESCENT = 2, BRC_STEPCAP = 3, BRC_OVERFLOW = 4, BRC_BADINJ = 5 };
/* BRC_EV_SEND: the first broadcast of (node, type, key) -- the reference harness's send log.
 * BRC_EV_COPY (connection-identity peers only): every later broadcast of it, one event each (the
 * :119 READY re-fires, repeated injected messages); with the SEND events they are the complete wire
 * traffic (wire.Codec.export).  Sender-identity peers suppress such duplicates on the network. */
enum { BRC_EV_DELIVER = 1, BRC_EV_DECIDE = 2, BRC_EV_SEND = 3, BRC_EV_COPY = 4 };

typedef struct {
    uint32_t n;               /* replicas per instance, self included (1..256) */
    uint32_t f;               /* fault bound: thresholds (n+f)/2, f+1, 2f+1, n-f+1.  Every value 0..n-1 is held to the
                               * oracle on every kernel (f >= n: BRC_E_INVALID, the reason names f): at 0 the slow set is
                               * empty, at n-1 one replica is fast, and once 2f+1 exceeds the honest replicas no READY
                               * quorum is reachable, so the reference and SPEC broadcasts deliver nothing */
    uint32_t protocol;        /* BRC_PROTO_* */
    uint32_t peer_mode;       /* BRC_PEER_SENDER / BRC_PEER_CONNECTION (core/brbroadcast.py:69-71) */
    uint64_t instances;       /* instances owned by this engine */
    uint64_t instance_offset; /* global id of instance 0 (Philox counter; multi-GPU shard) */
    uint64_t seed;            /* schedule seed (delays, proposals, slow set) */
    uint32_t delay_model;     /* BRC_DELAY_* */
    uint32_t delay_max;       /* D, 1..16 */
    uint32_t delay_const;     /* BRC_DELAY_CONST value */
    uint32_t round_cap;       /* consensus: instance DONE when every honest replica decided this many times */
    uint32_t step_cap;        /* last simulated step (<= 60000) */
    uint32_t key_window;      /* Q: live phase indices per origin (2, 4, 8; 16 .. 128 with n <= 64 and the
                                 reference / best-effort protocols, whose phase leakage keeps up to ~17
                                 phases of one origin in flight by round 8 and 127 by round 64 under
                                 slow-set D = 8; above 32 at n in 33..64 with sender peers, and
                                 Q * NV = 128 at n in 33..64 with connection peers: the key-lifetime
                                 kernel only; 16 and 32 at n > 64 with BRC_FLAG_WIDE_WINDOWS, below) */
    uint32_t variants;        /* NV: key variants per origin (1, 2 or 4; Q*NV <= 8, <= 128 where Q may be,
                                 <= 32 at n > 64 with BRC_FLAG_WIDE_WINDOWS) */
    uint32_t proposals;       /* BRC_PROPOSALS_* (consensus) */
    uint32_t byz_pattern;     /* BRC_BYZ_* applied to every instance */
    uint32_t event_capacity;  /* 0: no event log */
    uint64_t byzantine_mask;  /* replicas 0..63 that run no code (all instances; see brc_load_byzantine) */
    int32_t device;           /* HIP device ordinal */
    uint32_t mode;            /* BRC_MODE_* */
    uint64_t coin_seed;       /* BRC_MODE_SPEC: common-coin key */
    uint64_t byzantine_mask_hi[3];  /* replicas 64..255 that run no code */
    uint32_t flags;           /* BRC_FLAG_* */
    uint32_t reserved[3];
} brc_config;
/* BRC_FLAG_GENERAL_KEYS (v7): at n in 33..64 with sender peers and the reference protocol, run the
 * narrow kernel's general form instead of the lean one -- 8-B cells with generation tags, 3-bit value
 * ids (7 proposal strings besides "-1") and extra SENDs of one key (one payload SENT by several
 * origins, core/brbroadcast.py:74-79 keys by the payload string) -- what n <= 32 and connection peers
 * always have.  For the class API's single-instance clusters; the batched workloads keep the lean
 * kernels (4-B cells, 2-bit ids).
 * BRC_FLAG_WIDE_RECORDS (v8): at n > 64 with sender peers (any mode, either protocol), run the wide kernel's
 * instantiations that take records: restricted ECHO / READY (below) and extra SENDs of one key (brc_injection.dst_mask).
 * Opt-in: an engine without the flag launches the kernels it always did and refuses such records; with it the 4-waves-per-SIMD instantiations are not used and
 * every step tests one more word, so a run without records is slightly slower.  With n <= 64 or
 * connection peers brc_create fails with BRC_E_INVALID and a reason.
 * BRC_FLAG_WIDE_VALUES (v9): at n > 64 with sender peers, BRC_MODE_REFERENCE or BRC_MODE_BEB (either protocol), run
 * the wide kernel's instantiations that keep 3-bit value ids: value 0..7 in brc_injection (SEND, KEY,
 * BRC_INJ_DELIVER) and in brc_load_proposals, seven proposal strings besides "-1" as on the narrow kernels.  They are
 * the record form as well: such an engine accepts everything a BRC_FLAG_WIDE_RECORDS engine accepts, and the two
 * flags together select the same kernels.  Opt-in: an engine without the flag launches the kernels it always did
 * and refuses ids >= 4.  A replica's host masks of ids 4..7 stay in device memory rather than LDS, so binary
 * workloads cost what BRC_FLAG_WIDE_RECORDS costs and a delivery of such an id a few global accesses.
 * With n <= 64, connection peers or BRC_MODE_SPEC brc_create fails with BRC_E_INVALID and a reason.
 * BRC_FLAG_WIDE_WINDOWS (v10): at n > 64 with sender peers, BRC_MODE_REFERENCE or BRC_MODE_BEB (either protocol),
 * key_window * variants may be 16 or 32 besides what is accepted without the flag (<= 8).  The reference protocol's
 * phase leakage keeps more than 8 phases of one origin in flight from about its fourth round on (slow-set D = 8:
 * 11 by round 5, 18 by round 9), so without the flag such runs stop with BRC_OVERFLOW.  The kernels are the ones an
 * unflagged engine launches (their key-slot arithmetic is run-time); the flag lifts the host's limits, and a flagged
 * engine at key_window * variants <= 8 runs exactly what an unflagged one runs.  It combines with
 * BRC_FLAG_WIDE_RECORDS and BRC_FLAG_WIDE_VALUES.  Per instance the engine then holds NK * NPAD * 8 B of cells
 * (NK = NPAD * key_window * variants key slots, NPAD = 128 or 256): 2 / 4 MB at NPAD 128 and 8 / 16 MB at NPAD 256
 * for 16 / 32 slots per replica, plus 28 B (NPAD 128) or 44 B (NPAD 256) per key slot and the activity ring;
 * an allocation that does not fit fails brc_create with BRC_E_NOMEM and the size.  One workgroup's LDS is 37-42 /
 * 63-72 KB at NPAD 128 and 90-100 / 142-159 KB at NPAD 256, so three / two workgroups share a CU at NPAD 128 and
 * one at NPAD 256.  Refused with
 * BRC_E_INVALID and a reason: n <= 64 (the narrow kernels take windows up to 128 unflagged), BRC_MODE_SPEC (its
 * per-phase windows stay <= 8), connection peers (five words per cell: they keep key_window * variants <= 8),
 * key_window * variants > 32, and the one shape whose LDS carve exceeds a workgroup's 160 KB -- n > 128 with
 * key_window = 32 under uniform or geometric delays with delay_max > 8 (164,016 B; 16 x 2 and 8 x 4 variants fit).
 * BRC_FLAG_WIDE_LIFE (v11): at n > 64, run the wide key-lifetime kernel (csrc/brc_life_wide.h) instead of the wide
 * step kernel.  Under constant and slow-set delays a key's whole life is two receiver-class states (honest fast
 * receivers, honest slow ones), simulated in closed form when the key is created, so the engine keeps no cells: per
 * instance it holds 16 B * NPAD of consensus records and about 100 B, where the step kernel holds NK * NPAD * 8 B of
 * cells (4 / 8 / 16 MB at NPAD 256 for windows 8 / 16 / 32).  Such an engine is lifetime-only, like the engines at
 * n <= 64 whose step state does not fit (brc_last_kernel, below): brc_last_kernel reports BRC_KERNEL_LIFE before and
 * after the run; brc_inject, and brc_run with max_steps > 0, return BRC_E_UNSUPPORTED and name the kernel;
 * brc_reset, brc_reset_at, brc_load_proposals, brc_load_byzantine and every reader work as on any engine.  Results
 * are the step kernel's, field for field.  BRC_OVERFLOW when an origin's window is full (a SEND would reuse a slot
 * whose key still has arrivals ahead) or a replica starts more than min(key_window, 32) SENDs in one step, step-cap
 * stops (BRC_STEPCAP once the next step with arrivals lies past step_cap) and t_stop (the last step <= the stop at
 * which an honest cell had an arrival) behave as on the narrow key-lifetime kernel and the step kernels.
 * Eligible: sender peers, the consensus protocol, BRC_MODE_REFERENCE, BRC_MODE_SPEC (variants = 1) or BRC_MODE_BEB,
 * Philox or loaded proposals (value ids <= 3), BRC_DELAY_CONST or BRC_DELAY_SLOWSET with delay_max <= 8, no event
 * log, no byz_pattern (silent Byzantine replicas through byzantine_mask / byzantine_mask_hi / brc_load_byzantine),
 * key_window * variants <= 8, or 16 / 32 together with BRC_FLAG_WIDE_WINDOWS (REFERENCE / BEB).  One workgroup's LDS is
 * 16 / 24 / 38 KB at NPAD 128 and 47 / 62 / 91 KB at NPAD 256 for windows 8 / 16 / 32 (SPEC, window 8: 12 / 23 KB).
 * Anything else with the flag set fails brc_create with BRC_E_INVALID and a reason naming the field: n <= 64,
 * connection peers, the broadcast protocol, no proposals, uniform / geometric delays, delay_max > 8, an event log, a
 * pattern, BRC_FLAG_WIDE_RECORDS / BRC_FLAG_WIDE_VALUES (they select the step kernel's record / 3-bit forms), an LDS
 * carve above 160 KB, and BRC_KERNEL=step in the environment (a lifetime-only engine has no step state).  Without
 * the flag nothing changes: BRC_KERNEL=life at n > 64 still runs the step kernel.
 * BRC_FLAG_LIFE_PATTERN (v12): together with BRC_FLAG_WIDE_LIFE, byz_pattern = BRC_BYZ_EQUIVOCATE runs on the wide
 * key-lifetime kernel (its pattern form, csrc/brc_life_wide.h PAT).  The pattern is a function of the instance's
 * Byzantine mask: Byzantine replica b declares the keys (b * variants + v, s = 0) with value id 1 + v (v = 0, 1), SENDs
 * key 0 to the even replicas and key 1 to the odd ones at t = 0, and ECHOes and READYs both to everyone at t = 1.  The
 * kernel reads the mask itself and simulates such a key as four receiver-class states ((fast | slow) x (got the SEND |
 * did not)), so the engine keeps no injection list for the pattern; brc_load_byzantine (per-instance masks),
 * brc_reset, brc_reset_at, brc_load_proposals and every reader work, and the engine is lifetime-only like any
 * BRC_FLAG_WIDE_LIFE engine (brc_inject and stepped runs: BRC_E_UNSUPPORTED).  Results are those of an unflagged
 * engine running the pattern on the wide step kernel, field for field.  Eligible: everything BRC_FLAG_WIDE_LIFE
 * requires, BRC_MODE_REFERENCE or BRC_MODE_BEB, variants 2 or 4 (key_window * variants <= 8, or 16 / 32 with
 * BRC_FLAG_WIDE_WINDOWS).  One workgroup's LDS is BRC_FLAG_WIDE_LIFE's plus 16 B per 64 key slots and 64 B + 4 NPAD:
 * 16 / 23 / 37 KB at NPAD 128 and 48 / 62 / 90 KB at NPAD 256 for key_window * variants = 8 / 16 / 32 with variants = 2
 * (16,512 .. 91,776 B; a carve above 160 KB would be refused as under BRC_FLAG_WIDE_LIFE).  The flag set
 * on anything else fails brc_create with BRC_E_INVALID and a reason naming it: without BRC_FLAG_WIDE_LIFE, n <= 64 (a
 * pattern there runs on the step kernel, as it does at n in 33..64 whatever the flags), connection peers,
 * BRC_MODE_SPEC (variants = 1 above 64 replicas), byz_pattern = BRC_BYZ_NONE, variants = 1.  Without the flag nothing
 * changes: BRC_FLAG_WIDE_LIFE with a pattern is still refused.
 * BRC_FLAG_LIFE_VALUES (v13; bit 64 is unassigned and refused): together with BRC_FLAG_WIDE_LIFE, the wide key-lifetime
 * kernel keeps 3-bit consensus value ids (csrc/brc_life_wide.h V8): brc_load_proposals accepts ids 0..7 (seven proposal
 * strings besides "-1") and the run stays on the lifetime kernel; Philox proposals stay binary; decisions are read with
 * brc_read_value_decisions (brc_read_decisions: BRC_E_STATE once an id >= 4 was decided).  Results are those of a
 * BRC_FLAG_WIDE_VALUES engine on the wide step kernel, field for field; with binary proposals those of the
 * BRC_FLAG_WIDE_LIFE engine without the flag.  May be combined with BRC_FLAG_WIDE_WINDOWS and BRC_FLAG_LIFE_PATTERN
 * (the pattern's ids stay 1 and 2).  Eligible: everything BRC_FLAG_WIDE_LIFE requires, BRC_MODE_REFERENCE or
 * BRC_MODE_BEB.  One workgroup's LDS is BRC_FLAG_WIDE_LIFE's (or the pattern form's) plus one byte per key slot, the
 * slot's value id: + 1 / 2 / 4 KB at NPAD 128 and + 2 / 4 / 8 KB at NPAD 256 for key_window * variants = 8 / 16 / 32
 * (the largest carve: 100,928 B at NPAD 256, window 32).  Host-mask planes 0..3 stay in LDS; planes 4..7 live in device
 * memory, in a buffer of the wide step kernel's layout [instance][8][NPAD / 64][NPAD] u64 -- all eight planes are
 * allocated, NPAD^2 B per instance (16 KB at NPAD 128, 64 KB at NPAD 256), of which the kernel touches the upper half,
 * and only on a delivery that carries an id >= 4; brc_create, brc_reset and brc_reset_at zero it.  The flag set on
 * anything else fails brc_create with BRC_E_INVALID and a reason naming it: without BRC_FLAG_WIDE_LIFE, n <= 64,
 * connection peers, BRC_MODE_SPEC (its consensus is binary); with BRC_FLAG_WIDE_RECORDS / BRC_FLAG_WIDE_VALUES it is
 * refused as BRC_FLAG_WIDE_LIFE refuses them.  Without the flag nothing changes: a BRC_FLAG_WIDE_LIFE engine still
 * refuses id 4. */
enum { BRC_FLAG_GENERAL_KEYS = 1, BRC_FLAG_WIDE_RECORDS = 2, BRC_FLAG_WIDE_VALUES = 4, BRC_FLAG_WIDE_WINDOWS = 8,
       BRC_FLAG_WIDE_LIFE = 16, BRC_FLAG_LIFE_PATTERN = 32, BRC_FLAG_LIFE_VALUES = 128 };

/* Injections may arrive between brc_run calls.  A record's time must not lie before the step its instance's wave
 * item stands at (brc_instance_result.t_now once the engine has run): t < t_now is BRC_E_STATE.  t == t_now is
 * accepted: the next brc_run enters step t again for the new actions only -- no message of that step arrives or
 * is counted a second time -- and performs them after the actions step t has already seen.  An injection into a
 * QUIESCENT instance re-opens it (RUNNING); DONE, STEPCAP, OVERFLOW and BADINJ instances refuse (BRC_E_STATE).
 * A refused brc_inject call changes nothing, whatever valid records precede the refused one.
 * Extra-SEND and restricted ECHO / READY records (dst_mask below) leave their item's table when a later call adds
 * one to the same item and the record's last possible arrival, its time + delay_max, lies before the item's step:
 * only records in flight count against the 16.
 *
 * Restricted ECHO / READY: a BRC_INJ_MSG whose dst_mask is a proper subset of the n peers -- a faulty replica that
 * ECHOes or READYs a payload to part of the committee and stays silent towards the rest.  One message travels on
 * each link node -> d for d in dst_mask and arrives at t + delay(node, d); msgs_sent grows by the links used
 * (Byzantine destinations included).  Sender peers carry one (node, type, key) once per link: links an earlier
 * BRC_INJ_MSG of that (node, type, key) used are dropped from a later one (after a broadcast to every peer it
 * carries nothing and changes no counter; a broadcast after a restricted one goes over the remaining links).  One
 * BRC_EV_SEND event is logged, for the first link (node, type, key) ever uses, at that record's step.  The key must
 * exist (BRC_BADINJ otherwise, as for a message to every peer).
 *   Supported: the non-lean narrow step kernels with sender peers -- n <= 32, and n in 33..64 under
 *   BRC_FLAG_GENERAL_KEYS -- and the wide kernels (n > 64, sender peers) of an engine created with
 *   BRC_FLAG_WIDE_RECORDS, in every mode (REFERENCE, SPEC, BEB; broadcast and consensus; with or without an
 *   event log), from a node that is Byzantine in its instance (brc_config.byzantine_mask, or the mask
 *   brc_load_byzantine loaded).  On the wide kernels one workgroup is one instance: up to 16 records in flight per
 *   instance, over destination sets of up to 256 bits (dst_mask, dst_mask_hi).
 *   Documented rejections, each BRC_E_UNSUPPORTED with the kernel family named in brc_last_error: an honest
 *   sender (its own later broadcast would need per-link suppression the cells do not have); connection peers;
 *   the lean kernels (n in 33..64 with sender peers, no flag); the wide kernels (n > 64) without
 *   BRC_FLAG_WIDE_RECORDS; engines that run on the key-lifetime kernel only (they take no injection at all). */
typedef struct {
    uint32_t t;               /* action time: performed after step t, messages stamped t */
    uint16_t kind;            /* BRC_INJ_* */
    uint16_t type;            /* BRC_INJ_MSG: BRC_ECHO / BRC_READY */
    uint64_t instance;        /* engine-local instance index */
    uint32_t node;            /* proposer / sender */
    uint32_t kp;              /* key slot: origin * variants + variant */
    uint32_t s;               /* phase index 2*(round-1)+(phase-1), or BRB sequence */
    int32_t value;            /* value id (0 == "-1"): 0..7 on the narrow kernels that keep 3-bit ids
                                 (n <= 32, or connection peers at n <= 64; not BRC_MODE_SPEC) and on the
                                 wide kernels of an engine created with BRC_FLAG_WIDE_VALUES (n > 64,
                                 sender peers, not SPEC), 0..3 on the others (n in 33..64 with sender
                                 peers, n > 64 without the flag, SPEC); larger: BRC_E_INVALID.  The
                                 same range holds for brc_load_proposals */
    uint64_t dst_mask;        /* BRC_INJ_SEND / BRC_INJ_MSG destinations 0..63.  A second
                                 SEND of a key (another node, or the same again: one payload string
                                 SENT twice, one key in the reference) is an extra SEND on the
                                 narrow kernels that keep 3-bit value ids and, at n > 64 with sender
                                 peers, on an engine created with BRC_FLAG_WIDE_RECORDS (value ids
                                 stay 2 bits there) or BRC_FLAG_WIDE_VALUES.  It must not precede the key's first SEND
                                 (BRC_BADINJ for its instance), travels on the links of its
                                 destination set that its node has not used for a SEND of the key
                                 (sender peers; with none left it is accepted and changes nothing)
                                 and leaves the key's sender, send step, value and the first SEND's
                                 destination set as they are.  BRC_E_UNSUPPORTED on the others: the
                                 lean kernels, the wide kernels without the flag (connection peers
                                 above 64 cannot have it), lifetime-only engines.  A BRC_INJ_MSG
                                 to a proper subset of the peers (restricted ECHO / READY, below) is
                                 a record of the same table.  The table holds up to 16 records
                                 (extra SENDs and restricted ECHOs / READYs together) in flight per
                                 wave item (64 / NPAD instances, NPAD = n rounded up to 4, 8, 16,
                                 32, 64; n > 64 under BRC_FLAG_WIDE_RECORDS: per instance); one more:
                                 BRC_E_UNSUPPORTED, nothing changed */
    uint64_t dst_mask_hi[3];  /* destinations 64..255 (n > 64), as byzantine_mask_hi */
} brc_injection;

typedef struct {
    uint32_t status;          /* BRC_RUNNING ... */
    uint32_t t_stop;          /* last step with an arrival at an honest replica or an action */
    uint32_t t_now;           /* engine time of the instance's wave */
    uint32_t decided;         /* every honest replica decided at least once */
    uint64_t msgs_sent;       /* link messages sent (duplicate-suppressed) */
    uint64_t arrivals;        /* messages processed by honest replicas (replica-message-steps) */
    uint64_t cell_steps;      /* (receiver, key) cells that had arrivals, summed over steps */
    uint64_t deliveries;
} brc_instance_result;

typedef struct {
    uint32_t round, phase, value_count, decide_count;
    uint32_t first_decide_round, first_decide_t;
    int32_t first_decide_value, last_decide_value;
} brc_replica_result;

typedef struct {
    uint64_t instance;
    uint32_t t;
    uint8_t kind, node, type;
    uint8_t value;            /* value id of the key's payload (DECIDE: the decided value) */
    uint32_t a, b;            /* DELIVER: kp, s   DECIDE: round, value   SEND: kp, s */
} brc_event;

typedef struct {
    uint64_t instances, running, done, quiescent, stepcap, overflow, decided;
    uint64_t msgs_sent, arrivals, cell_steps, deliveries;
    uint64_t decide_rounds_sum;   /* sum of first-decide rounds over honest replicas */
    uint64_t max_t;
    uint64_t events_dropped;
    uint64_t lane_loads;          /* key-steps x lanes: one per real lane per processed key-step (lean kernels: wave-key-steps
                                     x 64; a key's first SEND key-step counts although it stores its row without loading it) */
} brc_stats;

int brc_create(const brc_config* cfg, void** engine);
int brc_load_proposals(void* engine, const int8_t* proposals /* [instances][n] value ids */);
/* Per-instance Byzantine masks: replaces the mask of every instance (brc_config.byzantine_mask is not ORed
 * in); bits at and above n are ignored; under BRC_BYZ_EQUIVOCATE the pattern is expanded again. */
int brc_load_byzantine(void* engine, const uint64_t* byz_masks /* [instances][(n + 63) / 64] */);
int brc_inject(void* engine, const brc_injection* list, size_t count);
int brc_run(void* engine, uint32_t max_steps, uint32_t* running_left);
/* Back to step 0 with no injections, for the same global instances (brc_reset_at: for others).  Nothing bounds
 * the number of resets, nor the KEY / SEND records injected over them: on the kernels whose cells carry a slot
 * generation tag (n <= 32, connection peers, BRC_FLAG_GENERAL_KEYS) the engine counts the allocations every epoch
 * can have made of one key slot and clears its cells fully, by itself, before a tag could come round.  Two things
 * remain within ONE epoch (reset to reset), where nothing can be cleared:
 *  - phase indices at or above s_limit = min(0x3FFE, (8188 - generations booked since the last full clear - extra
 *    records of the epoch) / passes * key_window) stop their instance with BRC_OVERFLOW (passes: PROPOSE records
 *    of one replica; below 6000 generations booked no full clear has happened yet, so s_limit can be as low as
 *    about 2188 * key_window);
 *  - brc_run is BRC_E_STATE ("slot generation budget exhausted") when the injected records of the epoch could
 *    advance one slot's tag past the generations left: on a fresh engine 8188 KEY records of one key (8187
 *    records of one slot under the consensus protocol), fewer after earlier epochs; brc_reset recovers. */
int brc_reset(void* engine);
int brc_read_instances(void* engine, uint64_t first, uint64_t count, brc_instance_result* out);
int brc_read_replicas(void* engine, uint64_t first, uint64_t count, brc_replica_result* out /* [count][n] */);
int brc_read_events(void* engine, brc_event* out, size_t cap, size_t* count);
int brc_read_stats(void* engine, brc_stats* out);
/* Decide-round histogram over instances (consensus): hist[r] = instances whose honest replicas
 * had ALL decided by round r (the max of their first-decide rounds), hist[0] = instances with an
 * undecided honest replica, rounds >= bins-1 in hist[bins-1].  bins in [2, 4096].  Per engine
 * (= per GPU shard); SURVEY §8(d) cfg5 all-reduces it over ranks (shard.reduce_stats). */
int brc_read_round_histogram(void* engine, uint64_t* hist, uint32_t bins);
/* Decisions of the honest replicas (consensus; the decide() upcall of
 * core/byzantinerandomizedconsensus.py:94): value_hist[v] for v = 0..3 counts replicas whose FIRST
 * decision carried value id v (0 is the reference's "-1"), value_hist[4] replicas that never
 * decided; *disagreements counts instances whose honest replicas' first decisions differ
 * (the agreement check of SURVEY §8(e)).  Per engine; shard.reduce_stats all-reduces them. */
int brc_read_decisions(void* engine, uint64_t* value_hist /* [5] */, uint64_t* disagreements);
/* The same over 3-bit value ids: value_hist[v] for v = 0..7, value_hist[8] never decided.
 * brc_read_decisions is BRC_E_STATE once a value id >= 4 was decided, on a narrow kernel or on an
 * engine created with BRC_FLAG_WIDE_VALUES alike: this call serves those. */
int brc_read_value_decisions(void* engine, uint64_t* value_hist /* [9] */, uint64_t* disagreements);
/* brc_reset, then re-key the engine to the global instances [instance_offset, +instances): one
 * engine sweeps a range larger than its device footprint in tiles, with the results one engine
 * over the whole range would give (every Philox counter uses the global id).  Loaded proposals
 * and Byzantine masks are kept (they are indexed by engine-local instance). */
int brc_reset_at(void* engine, uint64_t instance_offset);
/* Events first .. first+cap-1 of the log (brc_read_events reads from 0); *total = events logged
 * since the last reset, dropped ones included.  Lets a caller drain the log incrementally. */
int brc_read_events_range(void* engine, size_t first, brc_event* out, size_t cap, size_t* total);
int brc_last_kernel_ms(void* engine, float* ms);
/* Which kernel the last brc_run launched.  BRC_KERNEL_LIFE (the key-lifetime kernel) runs a fresh
 * engine (after brc_create / brc_reset) to completion in one launch when the configuration allows:
 * n in 33..64, consensus with Philox or loaded proposals, constant / slow-set delays with
 * delay_max <= 8 (its two-class form) or uniform / geometric delays with delay_max <= 16 (its
 * per-link form, which keeps a delivery-bitmap ring in HBM: 64 KB per instance at NK = 256, 128 KB
 * for delays above 8), no event log, no byz_pattern, no injections, max_steps == 0.  By default it
 * runs every such configuration except sender peers under uniform / geometric delays (the step kernel
 * is faster there); a run it cannot take (injections, max_steps > 0) goes to the step kernel.  Sender
 * peers whose step-kernel state (cells, slot arrays, activity ring) would exceed 90 % of the device's
 * TOTAL memory -- a choice fixed by the configuration and device model, not by what else holds memory
 * -- or whose key window is above 32 are lifetime-kernel-only, and so are connection peers at n in
 * 33..64 with Q * NV = 128 (8,192 key slots: the step kernel's LDS carve exceeds a workgroup's 160 KB):
 * brc_inject returns BRC_E_UNSUPPORTED and so does a run with max_steps > 0; where the lifetime kernel
 * cannot take such a configuration (BRC_KERNEL=step, an event log, ...) brc_create returns BRC_E_INVALID.  Before the first brc_run, brc_last_kernel reports the kernel a fresh run to
 * completion would launch.  The environment variable
 * BRC_KERNEL (read by brc_create) = life uses it for every eligible engine, = step never.  Its
 * results equal the step kernel's; its instances end final, so a later injection that would
 * re-open a QUIESCENT instance is BRC_E_STATE until brc_reset. */
enum { BRC_KERNEL_STEP = 0, BRC_KERNEL_LIFE = 1 };
int brc_last_kernel(void* engine, uint32_t* kind);
int brc_device_count(int* count);
const char* brc_last_error(void* engine);   /* engine NULL: why the last brc_create on this thread failed */
void brc_destroy(void* engine);
int brc_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
