"""VecEnv: the books of one engine as a batched environment for a policy that lives in torch, on the engine's GPU.

    import torch                                   # before the engine library is loaded: one HIP runtime per process
    from rl_markets_amd import engine
    from rl_markets_amd.vec_env import VecEnv

    env = VecEnv(eng)                              # eng: an engine.Engine with its events loaded
    obs = env.reset()                              # f32 [B, V], on the device
    while int(env.n_live) > 0:                     # (the one host read of the loop: ask every few steps, or not at all)
        actions = policy(obs).argmax(1).to(torch.int32)
        obs, reward, terminal, stepped = env.step(actions)

VecEnv(eng, book=True) also keeps the order book itself on the device (lob_vec_book): .levels f32 [B, 4, D] -- plane 0 ask prices, 1 ask
volumes, 2 bid prices, 3 bid volumes, level 0 the touch --, .own f32 [B, 16] (abi.OWN_*: inventory, the standing orders and their
queue positions, quotes, last action, PnL and reward sums, ticks) and .time_ms i64 [B], raw values as get_books() reports them.
They are attributes, refreshed behind every step() / observe() / reset() and ready wherever `obs` is.

VecEnv(eng, history=K) keeps the last K event records of every book on the device (lob_vec_history, 1 <= K <= abi.MAX_HISTORY):
.hist_levels f32 [B, K, 4, D] (the planes of .levels), .hist_trades f32 [B, K, 2, T] (plane 0 trade prices, 1 trade volumes),
.hist_time_ms i32 [B, K], oldest first with the record behind the current snapshot in slot K - 1 and zeros before the start of the
book's stream; .hist_valid i32 [B] counts the slots that hold a record and .hist_rec i32 [B] is the index of the newest one within
the book's stream (-1: none).  Refreshed like the book tensors; the two options are independent.

save(slot, mask) / restore(slot, mask) keep and put back the books' environment state on the device (lob_snapshot_save /
lob_snapshot_restore, 0 <= slot < abi.MAX_SNAPSHOTS): mask is a torch.bool or torch.uint8 tensor [B] on the engine's device (nonzero
selects the book), None every book.  A restored book continues exactly as it would have from the moment of the save; restore()
returns the refreshed `obs` (and refreshes the book / history tensors).  Per-book restarts on the same day:

    obs = env.reset(); env.save(0)                 # the state right after the reset
    ...
    obs = env.restore(0, mask=env.terminal != 0)   # the books that are over play their day again, the others carry on

A snapshot belongs to its episode (reset() voids it), and after a restore the engine's own learner calls (td_step, eval_step) are
refused until the next reset().  A VecEnv that never calls save() / restore() launches and allocates nothing for them.

act(mode) asks the engine's own tile-coded linear-Q agent (lob_vec_act): it returns .act_actions, int32 [B], the action its policy
takes on every book's latest observation -- "greedy" (what eval_step plays), "behaviour" (the learner's epsilon-greedy / Boltzmann
policy at the current epsilon / tau) or "argmax" (the first maximum, no random draw) --, and leaves the values it looked at in .act_q,
f64 [B, 9].  env.step(env.act()) is one agent step of the engine's greedy policy, with no host in it; it also works on books that
restore() has put back.  q_values(vars) evaluates the same weights on any f32 [n, V] tensor of states (lob_vec_q).  A VecEnv that
never calls act() allocates and launches nothing for it.

features() / tile_index() / update() open the agent's representation and its weights to a learner in torch (lob_vec_features,
lob_vec_update).  features() refreshes and returns .feat_sums, int32 [B, 96]: the action-independent hash sums of the 96 tiles (3
groups x 32 tilings) of every book's latest observation; features(vars) returns a fresh tensor for any f32 [n, V] states, and with
actions=... also the tile indices of that action per row, (sums, idx).  tile_index(sums, actions) is the contract in torch, in int64:
(sums + .tile_terms[group, action]) mod memory_size -- for all nine actions from the one [n, 96] tensor, 384 bytes per state.
update(step, actions, vars=None) adds step[s] to each of the 96 weights of (row s, actions[s]): the caller's whole per-tile amount
(for the learner's own rule pass alpha * delta / 32), on the engine's stream; act(), eval_step and td_step use the new weights in
the next call.

    sums = env.features()                                                    # [B, 96]
    q_sa = theta[env.tile_index(sums, a)].sum(-1)                            # Q(s, a) for any theta tensor a learner keeps
    env.update((alpha / 32) * (target - q_sa), a)                            # semi-gradient step on the engine's own weights

A VecEnv that calls none of the three allocates and launches nothing for them.

peek(actions=None) is the environment as a model (lob_vec_peek): for each of the nine actions -- or those listed -- what step() would
return had every book been given that action now, in .peek_obs f32 [9, B, V], .peek_reward f64 [9, B], .peek_terminal uint8 [9, B]
and .peek_stepped int32 [9, B] (plane a = action a; planes not asked for keep their last contents), in one launch, and the books
stay exactly where they are.  One-step expectimax targets under the engine's own weights:

    o, r, t, s = env.peek()
    q = env.q_values(o.view(9 * B, V)).view(9, B, 9).max(-1).values
    target = r + gamma * q * (t == 0)

On a ring-mode stream only with VecEnv(..., ring_lookahead=True) (below).  A VecEnv that never calls peek() allocates and launches nothing for it.

rollout(plans, gamma) is the same model several steps deep (lob_vec_rollout): the books rolled forward H steps under each of P
candidate plans per book, int32 [P, H, B] (or [P, H]: the same plan for every book), in one launch -- the reward of every step, the
observation and terminal behind the last, the steps that completed and the discounted return, as fresh tensors; the books stay
exactly where they are.  An action of -1 skips that step for that book: plans of unequal length.  On a ring-mode stream only with VecEnv(..., ring_lookahead=True) (below).
A VecEnv that never calls rollout() allocates and launches nothing for it.

branch(n) makes a branch set (lob_branch_fork): n private copies of every book's environment state that stay on the device between
calls and can be stepped one step at a time with actions a torch policy produces from their observations -- closed loop, where peek()
and rollout() need every action before the launch.  It returns a Branches object: .obs f32 [n, B, V], .reward f64 [n, B], .terminal
uint8 [n, B], .stepped int32 [n, B] are persistent tensors (overwritten by the next call: clone what must be kept); .step(actions)
steps every branch with actions int32 [n, B] (an action outside 0 .. 8 leaves that branch as it is: -1 steps a subset),
.select(parent) makes branch (i, b) a copy of branch (parent[i, b], b) as it stood, .fork() starts again from the books' present state
and .close() releases the set.  The books themselves stay exactly where they are and may step on meanwhile; reset() voids the set.
The return of the engine's own greedy policy over H steps from here:

    br = env.branch(n)
    ret = torch.zeros((n, B), dtype=torch.float64, device=dev)
    for h in range(H):
        a = env.q_values(br.obs.view(n * B, V)).argmax(-1).to(torch.int32).view(n, B)
        br.step(a)
        ret += gamma ** h * br.reward

Beam search over quote schedules, k beams per book: one set holds the beams' nine children each, and a round is one select() -- with
the parents a top-k gives -- and one step():

    br = env.branch(k * 9)
    child_action = (torch.arange(k * 9, device=dev) % 9).to(torch.int32).unsqueeze(1).expand(k * 9, B).contiguous()
    beam = torch.zeros((k, B), dtype=torch.int64, device=dev)              # the branches that hold the beams: all alike behind the fork
    ret = torch.zeros((k, B), dtype=torch.float64, device=dev)
    for h in range(H):
        br.select(beam.repeat_interleave(9, dim=0).to(torch.int32))        # branch i: a copy of beam i // 9 ...
        o, r, t, s = br.step(child_action)                                  # ... under action i % 9
        total = ret.repeat_interleave(9, dim=0) + gamma ** h * r
        value = env.q_values(o.view(k * 9 * B, V)).view(k * 9, B, 9).max(-1).values * (t == 0)
        beam = (total + gamma ** (h + 1) * value).topk(k, dim=0).indices    # the branches the next round descends from
        ret = total.gather(0, beam)

branch(n, book=True, history=K) also keeps the order book and the event window of every BRANCH on the device (lob_branch_book /
lob_branch_history): .levels f32 [n, B, 4, D], .own f32 [n, B, 16], .time_ms i64 [n, B] and .hist_levels f32 [n, B, K, 4, D],
.hist_trades f32 [n, B, K, 2, T], .hist_time_ms i32 [n, B, K], .hist_valid / .hist_rec i32 [n, B] -- per branch what the VecEnv's own
tensors of those names would hold had the books been in that branch's state, refreshed behind every fork() / step() / select().  A
torch network over the book and the window choosing the actions of a closed loop, where q_values() serves only the engine's own agent:

    br = env.branch(n, book=True, history=K)
    ret = torch.zeros((n, B), dtype=torch.float64, device=dev)
    for h in range(H):
        x = torch.cat([br.hist_levels.flatten(2), br.levels.flatten(2), br.own], dim=2)    # [n, B, K * 4 * D + 4 * D + 16]
        a = net(x.view(n * B, -1)).argmax(-1).to(torch.int32).view(n, B)
        br.step(a)
        ret += gamma ** h * br.reward

On a ring-mode stream only with VecEnv(..., ring_lookahead=True) (below).  A VecEnv that never calls branch() allocates and launches nothing for it, and a branch set
without the two options allocates and launches nothing for them.

VecEnv(eng, ..., ring_lookahead=True) switches peek(), rollout() and branch() on for a ring-mode stream (lob_look_ring; a stream of
more than LOB_TRACK_RING events, every recorded day).  There a cell's `terminal` may hold two more codes: abi.TERMINAL_AHEAD (3) -- the
step would have read beyond the window of the market track that is in memory; it is dropped (stepped 0, reward 0; a roll-out's plan ends
there for that book; a branch keeps its state and can be stepped again once the real books have stepped on) -- and, for a branch that
has been left far behind the real books, abi.TERMINAL_BEHIND (4): nothing is attempted until select() or fork() replaces it.  A
look-ahead may enqueue the track's refill in front of its launch.  .status() counts such cells in .ahead_cells / .behind_cells, and
.track_window() returns (lo, hi, complete), int32 numpy arrays [B]: the track entries [lo, hi) a look-ahead is served from (it waits).
Without the flag nothing changes and nothing new is launched or allocated; on a resident track the flag changes nothing.

step() reads the actions from the tensor's device memory and writes into five persistent tensors (lob_vec_step,
include/lob_engine.h): no copy to or from the host and no synchronisation.  The engine runs on a stream of its own; it is made
to wait for torch's current stream before the call (the actions are ready) and torch's current stream for the engine's after it
(the outputs are ready), both on the device.  The tensors are overwritten by the next step(): clone what must be kept.

torch is imported by this module only; nothing else under rl_markets_amd needs it."""
import torch

from . import abi


class VecEnv:
    def __init__(self, eng, book=False, history=0, ring_lookahead=False):
        self.eng = eng
        self.ahead_cells = self.behind_cells = 0
        if ring_lookahead:
            eng.look_ring(True)
        self.B, self.V = eng.B, eng.V
        dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.obs = torch.zeros((self.B, self.V), dtype=torch.float32, device=dev)
        self.reward = torch.zeros(self.B, dtype=torch.float64, device=dev)
        self.terminal = torch.zeros(self.B, dtype=torch.uint8, device=dev)
        self.stepped = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.n_live = torch.zeros(1, dtype=torch.int32, device=dev)
        self.out = abi.VecOut(self.obs.data_ptr(), self.reward.data_ptr(), self.terminal.data_ptr(), self.stepped.data_ptr(),
                              self.n_live.data_ptr())
        self.book_out = None
        if book:
            self.levels = torch.zeros((self.B, 4, eng.params.depth), dtype=torch.float32, device=dev)
            self.own = torch.zeros((self.B, abi.VEC_OWN_WORDS), dtype=torch.float32, device=dev)
            self.time_ms = torch.zeros(self.B, dtype=torch.int64, device=dev)
            self.book_out = abi.VecBookOut(self.levels.data_ptr(), self.own.data_ptr(), self.time_ms.data_ptr())
        self.history, self.hist_out = int(history), None
        if self.history:
            if not 1 <= self.history <= abi.MAX_HISTORY:
                raise ValueError("VecEnv: history must be 0 or 1 .. %d" % abi.MAX_HISTORY)
            K = self.history
            self.hist_levels = torch.zeros((self.B, K, 4, eng.params.depth), dtype=torch.float32, device=dev)
            self.hist_trades = torch.zeros((self.B, K, 2, eng.params.max_trades), dtype=torch.float32, device=dev)
            self.hist_time_ms = torch.zeros((self.B, K), dtype=torch.int32, device=dev)
            self.hist_valid = torch.zeros(self.B, dtype=torch.int32, device=dev)
            self.hist_rec = torch.zeros(self.B, dtype=torch.int32, device=dev)
            self.hist_out = abi.VecHistOut(self.hist_levels.data_ptr(), self.hist_trades.data_ptr(), self.hist_time_ms.data_ptr(),
                                           self.hist_valid.data_ptr(), self.hist_rec.data_ptr())
        self.act_actions = self.act_q = self.act_out = None   # (allocated by the first act())
        self.feat_sums = self._tile_terms = None   # (allocated by the first features() / tile_index())
        self.peek_obs = self.peek_reward = self.peek_terminal = self.peek_stepped = self.peek_out = None   # (allocated by the first peek())
        self.stream = torch.cuda.ExternalStream(eng.lob_stream(), device=dev)
        self.bad_actions = 0
        # (the zero fills above ran on torch's stream: the engine's first write must come after them)
        self.stream.wait_stream(torch.cuda.current_stream(dev))

    def _on_engine(self, fn, *args, inputs=()):
        """The hand-off between torch's current stream and the engine's, around one engine call; `inputs`: the caller's tensors the
        engine reads (None entries are skipped).  Output tensors are allocated or zero-filled before this is called."""
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)      # what torch has enqueued so far (the inputs, the zero fills, readers of the last outputs) comes first
        fn(*args)
        cur.wait_stream(self.stream)      # what torch enqueues from here on sees the outputs
        # The engine reads the inputs on its own stream, and the caching allocator must not hand their blocks out again before
        # that.  `cur` now waits for the engine's stream, so whatever follows on `cur` follows the read: the blocks are marked as
        # used on `cur` (nothing to do where they were allocated there), never on the engine's stream, which the allocator would
        # record an event on when a tensor is freed -- possibly after Engine.close() has destroyed that stream.
        for t in inputs:
            if t is not None:
                t.record_stream(cur)

    def _observing(self, fn, *args):
        fn(*args, self.out)
        if self.book_out is not None:
            self.eng.vec_book(self.book_out)   # (right behind it on the engine's stream: the book as the step left it)
        if self.hist_out is not None:
            self.eng.vec_history(self.history, self.hist_out)

    def _call(self, fn, *args, inputs=()):
        self._on_engine(self._observing, fn, *args, inputs=inputs)

    def reset(self):
        """lob_reset (which waits for its own result, as it always has) and the first observation."""
        self.eng.reset()
        return self.observe()

    def observe(self):
        """The observation without a step: after reset(), after the engine's clear_inventory()."""
        self._call(self.eng.vec_observe)
        return self.obs

    def step(self, actions):
        """actions: int32 [B] on the engine's device.  Returns (obs, reward, terminal, stepped), the persistent tensors."""
        if actions.dtype != torch.int32 or not actions.is_cuda or actions.shape != (self.B,) or not actions.is_contiguous():
            raise ValueError("VecEnv.step: actions must be a contiguous int32 CUDA tensor of shape (%d,)" % self.B)
        self._call(self.eng.vec_step, actions.data_ptr(), inputs=(actions,))
        return self.obs, self.reward, self.terminal, self.stepped

    _ACT_MODES = {"greedy": abi.ACT_GREEDY, "behaviour": abi.ACT_BEHAVIOUR, "argmax": abi.ACT_ARGMAX}

    def act(self, mode="greedy"):
        """lob_vec_act: the engine's own policy on every book's latest observation.  Returns .act_actions (int32 [B], persistent; 0
        for a book that is over); .act_q (f64 [B, 9]) holds the values it chose among.  "greedy" and "behaviour" draw from the books'
        own policy streams, as eval_step / td_step do; "argmax" draws nothing."""
        if mode not in self._ACT_MODES:
            raise ValueError("VecEnv.act: mode must be one of %s" % ", ".join(sorted(self._ACT_MODES)))
        if self.act_out is None:
            self.act_actions = torch.zeros(self.B, dtype=torch.int32, device=self.device)
            self.act_q = torch.zeros((self.B, abi.LOB_N_ACTIONS), dtype=torch.float64, device=self.device)
            self.act_out = abi.VecActOut(self.act_actions.data_ptr(), self.act_q.data_ptr())
        self._on_engine(self.eng.vec_act, self._ACT_MODES[mode], self.act_out)
        return self.act_actions

    def peek(self, actions=None):
        """lob_vec_peek: one-step look-ahead.  actions: an iterable of ints in 0 .. 8, None: all nine.  Returns (.peek_obs,
        .peek_reward, .peek_terminal, .peek_stepped), persistent tensors [9, B, V] / [9, B]: plane a holds what step() would return
        had every book been given action a now -- a book that is over: stepped 0, reward 0, its last observation; planes not asked
        for keep their last contents.  Nothing of the environment changes.  The expectimax recipe:

            o, r, t, s = env.peek()
            q = env.q_values(o.view(9 * B, V)).view(9, B, 9).max(-1).values
            target = r + gamma * q * (t == 0)
        """
        mask = abi.PEEK_ALL
        if actions is not None:
            mask = 0
            for a in actions:
                if int(a) != a or not 0 <= int(a) < abi.LOB_N_ACTIONS:
                    raise ValueError("VecEnv.peek: actions must be integers in 0 .. %d" % (abi.LOB_N_ACTIONS - 1))
                mask |= 1 << int(a)
            if mask == 0:
                raise ValueError("VecEnv.peek: no action given")
        if self.peek_out is None:
            n = abi.LOB_N_ACTIONS
            self.peek_obs = torch.zeros((n, self.B, self.V), dtype=torch.float32, device=self.device)
            self.peek_reward = torch.zeros((n, self.B), dtype=torch.float64, device=self.device)
            self.peek_terminal = torch.zeros((n, self.B), dtype=torch.uint8, device=self.device)
            self.peek_stepped = torch.zeros((n, self.B), dtype=torch.int32, device=self.device)
            self.peek_out = abi.VecPeekOut(self.peek_obs.data_ptr(), self.peek_reward.data_ptr(), self.peek_terminal.data_ptr(),
                                           self.peek_stepped.data_ptr())
        self._on_engine(self.eng.vec_peek, mask, self.peek_out)
        return self.peek_obs, self.peek_reward, self.peek_terminal, self.peek_stepped

    def rollout(self, plans, gamma=1.0):
        """lob_vec_rollout: multi-step look-ahead under action plans.  plans: a contiguous int32 CUDA tensor [P, H, B] on the
        engine's device, plans[p, h, b] the action of plan p at step h for book b (1 <= P <= abi.MAX_ROLLOUT_PLANS, 1 <= H <=
        abi.MAX_ROLLOUT_STEPS); [P, H]: the same plan for every book.  Returns fresh tensors (obs f32 [P, B, V], reward f64
        [P, H, B], terminal uint8 [P, B], stepped int32 [P, B], ret f64 [P, B]): what H consecutive step() calls would return from
        here under plan p -- every step's reward, obs and terminal behind the last step, the number of steps that completed, and
        ret = sum over h of gamma ** h * reward[p, h] (0 <= gamma <= 1).  A book that is over gives reward 0 and keeps its last
        observation; an action outside 0 .. 8 skips that step for that book and is not counted by status().  Nothing of the
        environment changes.  Random-shooting model-predictive control with the engine's own values at the leaves:

            plans = torch.randint(0, 9, (P, H, B), dtype=torch.int32, device=dev)
            o, r, t, n, ret = env.rollout(plans, gamma)
            tail = env.q_values(o.view(P * B, V)).view(P, B, 9).max(-1).values
            best = (ret + gamma ** H * tail * (t == 0)).argmax(0)
            env.step(plans[best, 0, torch.arange(B, device=dev)].contiguous())
        """
        if (not isinstance(plans, torch.Tensor) or plans.dtype != torch.int32 or not plans.is_cuda or plans.device != self.device
                or plans.dim() not in (2, 3) or (plans.dim() == 3 and plans.shape[2] != self.B) or not plans.is_contiguous()
                or not 1 <= plans.shape[0] <= abi.MAX_ROLLOUT_PLANS or not 1 <= plans.shape[1] <= abi.MAX_ROLLOUT_STEPS):
            raise ValueError("VecEnv.rollout: plans must be a contiguous int32 CUDA tensor of shape (P, H, %d) or (P, H) on the engine's device, "
                             "1 <= P <= %d, 1 <= H <= %d" % (self.B, abi.MAX_ROLLOUT_PLANS, abi.MAX_ROLLOUT_STEPS))
        gamma = float(gamma)
        if not 0.0 <= gamma <= 1.0:
            raise ValueError("VecEnv.rollout: gamma must lie in [0, 1]")
        P, H = int(plans.shape[0]), int(plans.shape[1])
        if plans.dim() == 2:
            plans = plans.unsqueeze(2).expand(P, H, self.B).contiguous()
        obs = torch.empty((P, self.B, self.V), dtype=torch.float32, device=self.device)
        reward = torch.empty((P, H, self.B), dtype=torch.float64, device=self.device)
        terminal = torch.empty((P, self.B), dtype=torch.uint8, device=self.device)
        stepped = torch.empty((P, self.B), dtype=torch.int32, device=self.device)
        ret = torch.empty((P, self.B), dtype=torch.float64, device=self.device)
        out = abi.VecRolloutOut(obs.data_ptr(), reward.data_ptr(), terminal.data_ptr(), stepped.data_ptr(), ret.data_ptr())
        self._on_engine(self.eng.vec_rollout, plans.data_ptr(), P, H, gamma, out, inputs=(plans,))
        return obs, reward, terminal, stepped, ret

    def branch(self, n, book=False, history=0):
        """lob_branch_fork: the engine's branch set (one per engine) remade as n (1 .. abi.MAX_BRANCHES) copies of every book's
        present state.  Returns a Branches object (its tensors are allocated here, the engine's buffers by the engine: the first
        fork, and one that needs more room than any before, synchronises the device).  book / history (0 .. abi.MAX_HISTORY): the
        set also keeps every branch's order book / last `history` event records on the device (Branches)."""
        return Branches(self, n, book=book, history=history)

    def q_values(self, vars):
        """lob_vec_q: Q(s, .) under the engine's weights (theta; book 0's under private theta) for n free-standing states, f32 [n, V]
        on the engine's device -> a new f64 [n, 9] tensor; bit for bit Engine.q_values of the same rows."""
        n = self._rows(vars, "q_values")
        q = torch.empty((n, abi.LOB_N_ACTIONS), dtype=torch.float64, device=self.device)
        self._on_engine(self.eng.vec_q, vars.data_ptr(), n, q.data_ptr(), inputs=(vars,))
        return q

    @property
    def tile_terms(self):
        """lob_vec_terms: the action terms of the tile hash, int64 [3, 9] (group, action) on the device, reduced mod memory_size;
        made on first use."""
        if self._tile_terms is None:
            self._tile_terms = torch.tensor(self.eng.vec_terms(), dtype=torch.int64, device=self.device)
        return self._tile_terms

    def _rows(self, vars, who):
        if (not isinstance(vars, torch.Tensor) or vars.dtype != torch.float32 or not vars.is_cuda or vars.device != self.device
                or vars.dim() != 2 or vars.shape[1] != self.V or vars.shape[0] < 1 or not vars.is_contiguous()):
            raise ValueError("VecEnv.%s: vars must be a contiguous float32 CUDA tensor of shape (n, %d) on the engine's device" % (who, self.V))
        return vars.shape[0]

    def _vec(self, t, dtype, n, who, what):
        if (not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or t.device != self.device or t.shape != (n,)
                or not t.is_contiguous()):
            raise ValueError("VecEnv.%s: %s must be a contiguous %s CUDA tensor of shape (%d,) on the engine's device"
                             % (who, what, str(dtype).replace("torch.", ""), n))

    def features(self, vars=None, actions=None):
        """lob_vec_features: the hash sums of the 96 tiles of every state, int32 [n, 96].  vars None: the books' latest observation,
        into the persistent .feat_sums (overwritten by the next call: clone what must be kept); else f32 [n, V] states and a fresh
        tensor.  With actions (int32 [n]) it returns (sums, idx): idx int32 [n, 96], fresh, the tile indices of that action per row
        (-1 throughout a row whose action is out of range) -- tile_index(sums, actions) without the gather."""
        n = self.B if vars is None else self._rows(vars, "features")
        if actions is not None:
            self._vec(actions, torch.int32, n, "features", "actions")
        if vars is None:
            if self.feat_sums is None:
                self.feat_sums = torch.zeros((self.B, abi.N_TILES), dtype=torch.int32, device=self.device)
            sums = self.feat_sums
        else:
            sums = torch.empty((n, abi.N_TILES), dtype=torch.int32, device=self.device)
        idx = None if actions is None else torch.empty((n, abi.N_TILES), dtype=torch.int32, device=self.device)
        self._on_engine(self.eng.vec_features, None if vars is None else vars.data_ptr(), n, None if actions is None else actions.data_ptr(),
                        abi.VecFeatOut(sums.data_ptr(), None if idx is None else idx.data_ptr()), inputs=(vars, actions))
        return sums if actions is None else (sums, idx)

    def tile_index(self, sums, actions):
        """The contract of lob_vec_features in torch: (sums[s, p] + tile_terms[p // 32, actions[s]]) mod memory_size, int64 [n, 96]
        -- the weights of (row s, actions[s]); Engine.features' [s, a, :] for a = actions[s].  actions: integers in 0 .. 8, [n]."""
        terms = self.tile_terms[:, actions.long()].t().repeat_interleave(32, dim=1)   # [n, 96]
        return (sums.long() + terms) % int(self.eng.M)

    def update(self, step, actions, vars=None, second=False):
        """lob_vec_update: theta[tile] += step[s] over the 96 tiles of (row s, actions[s]); step f64 [n], actions int32 [n]; vars None:
        the books' latest observation (n = B; under private theta book s's own vector), else f32 [n, V] states (book 0's vector under
        private theta).  second: theta_b (double Q only).  A row with step 0.0 writes nothing; a row whose action is out of range is
        skipped and counted (status())."""
        n = self.B if vars is None else self._rows(vars, "update")
        self._vec(step, torch.float64, n, "update", "step")
        self._vec(actions, torch.int32, n, "update", "actions")
        self._on_engine(self.eng.vec_update, None if vars is None else vars.data_ptr(), n, actions.data_ptr(), step.data_ptr(), second,
                        inputs=(step, actions, vars))

    def _mask_ptr(self, mask, who):
        if mask is None:
            return None
        if (not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool) or not mask.is_cuda or mask.device != self.device
                or mask.shape != (self.B,) or not mask.is_contiguous()):
            raise ValueError("VecEnv.%s: mask must be a contiguous uint8 or bool CUDA tensor of shape (%d,) on the engine's device" % (who, self.B))
        return mask.data_ptr()

    def save(self, slot=0, mask=None):
        """lob_snapshot_save: the environment state of the selected books (mask None: all, which (re)starts the slot) into `slot`.
        The slot's first save allocates its buffer and with that synchronises the device; later ones only enqueue."""
        ptr = self._mask_ptr(mask, "save")
        self._on_engine(self.eng.snapshot_save, slot, ptr, inputs=(mask,))

    def _restore_observe(self, slot, ptr, out):
        self.eng.snapshot_restore(slot, ptr)
        self.eng.vec_observe(out)

    def restore(self, slot=0, mask=None):
        """lob_snapshot_restore of the selected books from `slot`, then the observation (and the book / history tensors) of the
        batch as it now stands.  Returns obs."""
        ptr = self._mask_ptr(mask, "restore")
        self._call(self._restore_observe, slot, ptr, inputs=(mask,))
        return self.obs

    def status(self):
        """lob_vec_status: waits once; LOB_OK, or LOB_EINVAL when actions were out of range since the last call (their number
        is left in .bad_actions).  A malformed event stream raises engine.LobError (LOB_EDATA).  .ahead_cells / .behind_cells: the
        look-aheads' cells of abi.TERMINAL_AHEAD / abi.TERMINAL_BEHIND since the last call (ring_lookahead=True; else 0)."""
        rc, self.bad_actions = self.eng.vec_status()
        self.ahead_cells, self.behind_cells = self.eng.look_counts()
        return rc

    def track_window(self):
        """lob_track_window: (lo, hi, complete), int32 numpy arrays [B].  Waits for the engine's stream: for diagnostics and tests."""
        return self.eng.track_window()


class Branches:
    """A branch set of a VecEnv (VecEnv.branch): n private copies of every book's environment state, stepped and rearranged on the
    device.  The engine holds one set: making another Branches, or fork() with it, remakes that set.

    book=True: .levels f32 [n, B, 4, D], .own f32 [n, B, 16] and .time_ms i64 [n, B] (lob_branch_book); history=K (1 ..
    abi.MAX_HISTORY): .hist_levels f32 [n, B, K, 4, D], .hist_trades f32 [n, B, K, 2, T], .hist_time_ms i32 [n, B, K], .hist_valid
    and .hist_rec i32 [n, B] (lob_branch_history) -- [i, b] is what the VecEnv's tensor of that name would hold at [b] had the books
    been in branch i's state.  Persistent tensors, refreshed right behind every fork(), step() and select() on the engine's stream,
    ready wherever .obs is.  Without the options the attributes do not exist and nothing is allocated or launched for them.  A
    network over the book and the window driving a closed loop:

        br = env.branch(n, book=True, history=K)
        for h in range(H):
            x = torch.cat([br.hist_levels.flatten(2), br.levels.flatten(2), br.own], dim=2)
            br.step(net(x.view(n * B, -1)).argmax(-1).to(torch.int32).view(n, B))
    """

    def __init__(self, env, n, book=False, history=0):
        if int(n) != n or not 1 <= int(n) <= abi.MAX_BRANCHES:
            raise ValueError("VecEnv.branch: n must be an integer in 1 .. %d" % abi.MAX_BRANCHES)
        self.history = int(history)
        if int(history) != history or not 0 <= self.history <= abi.MAX_HISTORY:
            raise ValueError("VecEnv.branch: history must be 0 or 1 .. %d" % abi.MAX_HISTORY)
        self.env, self.n = env, int(n)
        N, B, V, dev = self.n, env.B, env.V, env.device
        self.obs = torch.zeros((N, B, V), dtype=torch.float32, device=dev)
        self.reward = torch.zeros((N, B), dtype=torch.float64, device=dev)
        self.terminal = torch.zeros((N, B), dtype=torch.uint8, device=dev)
        self.stepped = torch.zeros((N, B), dtype=torch.int32, device=dev)
        self.out = abi.BranchOut(self.obs.data_ptr(), self.reward.data_ptr(), self.terminal.data_ptr(), self.stepped.data_ptr())
        self.book_out = self.hist_out = None
        D, T = env.eng.params.depth, env.eng.params.max_trades
        if book:
            self.levels = torch.zeros((N, B, 4, D), dtype=torch.float32, device=dev)
            self.own = torch.zeros((N, B, abi.VEC_OWN_WORDS), dtype=torch.float32, device=dev)
            self.time_ms = torch.zeros((N, B), dtype=torch.int64, device=dev)
            self.book_out = abi.VecBookOut(self.levels.data_ptr(), self.own.data_ptr(), self.time_ms.data_ptr())
        if self.history:
            K = self.history
            self.hist_levels = torch.zeros((N, B, K, 4, D), dtype=torch.float32, device=dev)
            self.hist_trades = torch.zeros((N, B, K, 2, T), dtype=torch.float32, device=dev)
            self.hist_time_ms = torch.zeros((N, B, K), dtype=torch.int32, device=dev)
            self.hist_valid = torch.zeros((N, B), dtype=torch.int32, device=dev)
            self.hist_rec = torch.zeros((N, B), dtype=torch.int32, device=dev)
            self.hist_out = abi.VecHistOut(self.hist_levels.data_ptr(), self.hist_trades.data_ptr(), self.hist_time_ms.data_ptr(),
                                           self.hist_valid.data_ptr(), self.hist_rec.data_ptr())
        self.fork()

    def _observing(self, fn, *args):
        fn(*args)
        if self.book_out is not None:
            self.env.eng.branch_book(self.book_out)   # (right behind it on the engine's stream: the branches as the call left them)
        if self.hist_out is not None:
            self.env.eng.branch_history(self.history, self.hist_out)

    def _call(self, fn, *args, inputs=()):
        self.env._on_engine(self._observing, fn, *args, inputs=inputs)

    def _words(self, t, who, what):
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or not t.is_cuda or t.device != self.env.device
                or t.shape != (self.n, self.env.B) or not t.is_contiguous()):
            raise ValueError("Branches.%s: %s must be a contiguous int32 CUDA tensor of shape (%d, %d) on the engine's device"
                             % (who, what, self.n, self.env.B))

    def fork(self):
        """lob_branch_fork again: every branch becomes a copy of its book's present state.  Returns (obs, reward, terminal, stepped):
        the books' latest observation and terminal word in every plane, reward 0, stepped 0."""
        self._call(self.env.eng.branch_fork, self.n, self.out)
        return self.obs, self.reward, self.terminal, self.stepped

    def step(self, actions):
        """lob_branch_step: actions int32 [n, B] on the engine's device.  Returns (obs, reward, terminal, stepped), the persistent
        tensors: per branch what VecEnv.step would return had the books been in that branch's state."""
        self._words(actions, "step", "actions")
        self._call(self.env.eng.branch_step, actions.data_ptr(), self.out, inputs=(actions,))
        return self.obs, self.reward, self.terminal, self.stepped

    def select(self, parent):
        """lob_branch_select: parent int32 [n, B]; branch (i, b) becomes a copy of branch (parent[i, b], b) as it stood before the
        call (outside 0 .. n - 1: it keeps itself).  Returns (obs, terminal) of the new arrangement; .reward and .stepped keep the
        last step's values in the old arrangement."""
        self._words(parent, "select", "parent")
        self._call(self.env.eng.branch_select, parent.data_ptr(), self.out, inputs=(parent,))
        return self.obs, self.terminal

    def close(self):
        """lob_branch_close: releases the engine's buffers of the set (waits for the engine's stream)."""
        self.env.eng.branch_close()
