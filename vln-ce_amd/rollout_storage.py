"""The DD-PPO rollout storage on the device: a drop-in for
`ActionDictRolloutStorage` of vlnce_baselines/common/rollout_storage.py.  The arenas are the
reference's torch tensors, with its shapes, dtypes and attribute names -- the trainer indexes them
directly (`rollouts.observations[k][rollouts.step]`, ddppo_waypoint_trainer.py:162-173, 289-298,
394-395) -- and `step` is a host int.  What changes is who moves the rows:

    insert              ~17 copy_ launches          -> one vlnce_rollout_copy
    after_update        ~11 copy_ launches          -> one vlnce_rollout_copy
    recurrent_generator a Python loop over the environments, ~25 stack / view launches per
                        minibatch                   -> one vlnce_rollout_gather per minibatch
    get_advantages      a mean() / std() chain (WDDPPO.get_advantages, ddppo_alg.py:30-35)
                                                    -> one vlnce_ppo_advantages
    compute_returns     a Python loop over the steps -> vlnce_ppo_returns

None of them synchronises with the host; the reference's NaN assertion inside compute_returns, which
does, is `check_returns()` here, on demand.  Nothing fails on a dtype or a layout: a source the
kernel does not convert goes through `Tensor.copy_`, a source whose rows are not contiguous inside
is made contiguous first (a source with only a row stride -- a crop handed out as a view -- is read
as it is).
"""
import math

import torch

from . import _lib
from ._lib import ROLLOUT_MAX_ENVS, ROLLOUT_MAX_FIELDS, RolloutCopyField, RolloutGatherField

ACTION_KEYS = ("pano", "offset", "distance")
FRAME_KEYS = ("rgb", "depth", "rgb_history", "depth_history")   # what the trunk-feature arenas stand in for
EPS_PPO = 1e-5   # ddppo_alg.py:35


def _L():
    return _lib.get_lib()


def _row_source(t, E):
    """t [n, ...] as (tensor, row stride in elements) with every row contiguous inside"""
    expect = 1
    for size, stride in zip(reversed(t.shape[1:]), reversed(t.stride()[1:])):
        if size != 1 and stride != expect:
            t = t.contiguous()
            break
        expect *= size
    return t, (int(t.stride(0)) if t.size(0) > 1 else E)


def _split(seq, n):
    return [seq[i:i + n] for i in range(0, len(seq), n)]


class ActionDictRolloutStorage:
    """A RolloutStorage container for actions consisting of pano, offset, and distance components.
    `device=` allocates the arenas where they will live (at full size they are ~1.4 GB: filling them
    on the host and moving them is a waste); `.to(device)` works as in the reference.

    `trunk_features={"rgb": shape, "depth": shape}` (WaypointPredictionNet.trunk_feature_shapes()) adds
    the arenas of the trunk-feature cache to `observations`: `<sensor>_features` [T+1, N, P, *shape] and
    `<sensor>_history_features` [T+1, N, *shape], the outputs of the frozen visual trunks for the
    frames beside them.  As observations they are carried by after_update and cut into minibatches
    with everything else.  `trunk_valid[row]` says whether row's `<sensor>_features` were written
    (ppo_harness.act_for_rollout / bootstrap_value do that), `trunk_key` under which
    trunk_cache_key() of the net."""

    def __init__(self, num_steps, num_envs, observation_space, recurrent_hidden_state_size,
                 num_recurrent_layers=1, continuous_offset=True, continuous_distance=True, *,
                 device=None, trunk_features=None):
        def zeros(*shape, dtype=torch.float32):
            return torch.zeros(*shape, dtype=dtype, device=device)

        self.observations = {}
        for sensor in observation_space.spaces:
            self.observations[sensor] = zeros(num_steps + 1, num_envs,
                                              *observation_space.spaces[sensor].shape)
        self.has_trunk_features = trunk_features is not None
        self.trunk_valid = [False] * (num_steps + 1)
        self.trunk_key = None
        if trunk_features is not None:
            for sensor in ("rgb", "depth"):
                P = observation_space.spaces[sensor].shape[0]
                shape = tuple(trunk_features[sensor])
                self.observations[sensor + "_features"] = zeros(num_steps + 1, num_envs, P, *shape)
                self.observations[sensor + "_history_features"] = zeros(num_steps + 1, num_envs, *shape)
        self.recurrent_hidden_states = zeros(num_steps + 1, num_envs, num_recurrent_layers,
                                             recurrent_hidden_state_size)
        self.rewards = zeros(num_steps, num_envs, 1)
        self.value_preds = zeros(num_steps + 1, num_envs, 1)
        self.returns = zeros(num_steps + 1, num_envs, 1)
        self.action_log_probs = zeros(num_steps, num_envs, 1)
        self.actions = {k: zeros(num_steps, num_envs, 1) for k in ACTION_KEYS}
        discrete = {"pano": True, "offset": not continuous_offset, "distance": not continuous_distance}
        self.prev_actions = {k: zeros(num_steps + 1, num_envs, 1,
                                      dtype=torch.int64 if discrete[k] else torch.float32)
                             for k in ACTION_KEYS}
        self.masks = zeros(num_steps + 1, num_envs, 1, dtype=torch.uint8)
        self.num_steps = num_steps
        self.step = 0
        self._gae = None   # (gamma, tau) of the last compute_returns under GAE, for check_returns
        self._build_tables()

    # ---- field tables: which arenas after_update carries over and a minibatch is cut from
    def _build_tables(self):
        self._carried = (list(self.observations.values()) + [self.recurrent_hidden_states, self.masks]
                         + [self.prev_actions[k] for k in self.prev_actions])
        # (arena, once) in the order of the yielded tuple's tensors; the advantages join per call
        self._batched = ([(a, False) for a in self.observations.values()]
                         + [(self.recurrent_hidden_states, True)]
                         + [(self.actions[k], False) for k in self.actions]
                         + [(self.prev_actions[k], False) for k in self.actions]
                         + [(a, False) for a in (self.value_preds, self.returns, self.masks,
                                                 self.action_log_probs)])
        self._row_views = {}                       # (id(arena), row) -> arena[row]
        self._pairs_of, self._pairs = None, {}     # the library asked, {(src dtype, dst dtype): converts}

    def to(self, device):
        for sensor in self.observations:
            self.observations[sensor] = self.observations[sensor].to(device)
        self.recurrent_hidden_states = self.recurrent_hidden_states.to(device)
        self.rewards = self.rewards.to(device)
        self.value_preds = self.value_preds.to(device)
        self.returns = self.returns.to(device)
        for k in self.actions:
            self.actions[k] = self.actions[k].to(device)
            self.prev_actions[k] = self.prev_actions[k].to(device)
        self.action_log_probs = self.action_log_probs.to(device)
        self.masks = self.masks.to(device)
        self._build_tables()

    # ---- row blocks: [(arena, row, source)] -> arena[row] in one launch
    def _row(self, arena, r):
        """arena[r], made once per (arena, row): an insert builds no views of its own.  (A view keeps
        its base tensor alive, so the key cannot come to name another tensor.)"""
        key = (id(arena), r)
        view = self._row_views.get(key)
        if view is None:
            view = self._row_views[key] = arena[r]
        return view

    def _converts(self, lib, src_dtype, dst_dtype):
        if lib is not self._pairs_of:
            self._pairs_of, self._pairs = lib, {}
        ok = self._pairs.get((src_dtype, dst_dtype))
        if ok is None:
            ok = self._pairs[src_dtype, dst_dtype] = lib.rollout_copy_supported(src_dtype, dst_dtype)
        return ok

    def _copy_rows(self, triples):
        lib, fields = _L(), []
        for arena, r, src in triples:
            dst = self._row(arena, r)
            if (not torch.is_tensor(src) or src.device != dst.device or src.shape != dst.shape
                    or not self._converts(lib, src.dtype, dst.dtype)):
                dst.copy_(torch.as_tensor(src))   # broadcasts, converts and refuses as the reference does
                continue
            E = arena.stride(0) // max(arena.size(1), 1)   # (the arenas are contiguous)
            if E == 0:
                continue
            stride = E
            if not src.is_contiguous():
                src, stride = _row_source(src, E)
            fields.append(RolloutCopyField(src, dst, E, stride, E))
        n_rows = self.rewards.size(1)
        for part in _split(fields, ROLLOUT_MAX_FIELDS):
            lib.rollout_copy(part, n_rows)

    def insert(self, observations, recurrent_hidden_states, action, action_log_probs, value_preds,
               rewards, masks):
        s = self.step
        triples = [(self.observations[sensor], s + 1, observations[sensor]) for sensor in observations]
        triples.append((self.recurrent_hidden_states, s + 1, recurrent_hidden_states))
        for k in action:
            triples.append((self.actions[k], s, action[k]))
            triples.append((self.prev_actions[k], s + 1, action[k]))
        triples += [(self.action_log_probs, s, action_log_probs), (self.value_preds, s, value_preds),
                    (self.rewards, s, rewards), (self.masks, s + 1, masks)]
        self._copy_rows(triples)
        self.trunk_valid[s + 1] = False   # (the row's frames are new; its features are not written yet)
        self.step = s + 1

    def after_update(self):
        if self.step != 0:   # (row 0 onto itself: nothing to move)
            self._copy_rows([(a, 0, self._row(a, self.step)) for a in self._carried])
        self.trunk_valid = [self.trunk_valid[self.step]] + [False] * self.num_steps   # the flag moves with its row
        self.step = 0

    def compute_returns(self, next_value, use_gae, gamma, tau):
        """rollout_storage.py:127-152 over rows [0, step] in one launch: writes `returns`, and
        `value_preds[step]` under GAE.  The NaN assertion of the reference is check_returns()."""
        T, N = self.step, self.rewards.size(1)
        self._gae = (gamma, tau) if use_gae else None
        if T == 0:   # no step to walk: only the bootstrap row is set
            (self.value_preds if use_gae else self.returns)[0] = next_value
            return
        nv = next_value.to(device=self.returns.device, dtype=torch.float32).contiguous()
        _L().ppo_returns(self.rewards, self.value_preds, self.masks[:T + 1].float(), nv, self.returns,
                         T, N, gamma, tau, use_gae)

    def check_returns(self):
        """the reference's assertion on the returns (rollout_storage.py:141-145), on demand: the one
        call of this class that waits for the device"""
        T = self.step
        if T == 0 or not bool(torch.isnan(self.returns[:T]).any()):
            return
        if self._gae is None:
            raise AssertionError("Return is NaN.")
        gamma, tau = self._gae
        gae = 0
        for step in reversed(range(T)):   # the reference's walk, to report the step it would have
            delta = (self.rewards[step] + gamma * self.value_preds[step + 1] * self.masks[step + 1]
                     - self.value_preds[step])
            gae = delta + gamma * tau * self.masks[step + 1] * gae
            if torch.isnan(gae + self.value_preds[step]).any():
                raise AssertionError(f"Return is NaN.\nreward:\t{self.rewards[step]}"
                                     f"\ngae:\t{gae}\ndelta:\t{delta}"
                                     f"\nvalue_preds: {self.value_preds[step]}")
        raise AssertionError("Return is NaN.")

    def get_advantages(self, use_normalized_advantage=False):
        """WDDPPO.get_advantages (ddppo_alg.py:30-35) over the `step` rows collected: [step, N, 1]"""
        T, N = self.step, self.rewards.size(1)
        adv = torch.empty((T, N, 1), dtype=torch.float32, device=self.returns.device)
        if T > 0:
            _L().ppo_advantages(self.returns, self.value_preds, adv, T, N, use_normalized_advantage,
                                EPS_PPO)
        return adv

    def trunk_rows_valid(self, key):
        """whether every collected row [0, step) holds trunk features made under `key`"""
        return (self.has_trunk_features and self.trunk_key is not None and self.trunk_key == key
                and all(self.trunk_valid[:self.step]))

    def recurrent_generator(self, advantages, num_mini_batch, frames=True):
        """The yielded `actions_batch` and `prev_actions_batch` are dictionaries with keys
        ["pano", "offset", "distance"] whose values are batched action elements.  Rows are
        time-major, t * N' + j.  frames=False leaves the raw-frame arenas (FRAME_KEYS) out of the
        gather and out of the yielded observations: the trunk-feature arenas stand in for them."""
        num_processes = self.rewards.size(1)
        assert num_processes >= num_mini_batch, (
            "Trainer requires the number of processes ({}) "
            "to be greater than or equal to the number of "
            "trainer mini batches ({}).".format(num_processes, num_mini_batch)
        )
        num_envs_per_batch = num_processes // num_mini_batch
        perm = torch.randperm(num_processes)
        T, dev = self.step, self.returns.device
        adv = advantages.to(dev).contiguous()
        sensors = [k for k in self.observations if frames or k not in FRAME_KEYS]
        arenas = self._batched + [(adv, False)]
        if not frames:
            assert self.has_trunk_features, "frames=False needs the trunk-feature arenas"
            arenas = [(self.observations[k], False) for k in sensors] + arenas[len(self.observations):]
        lib = _L()
        for start_ind in range(0, num_processes, num_envs_per_batch):
            # (an indivisible count ends as the reference does: IndexError behind the full batches)
            envs = [int(perm[start_ind + offset]) for offset in range(num_envs_per_batch)]
            n, outs, fields = len(envs), [], []
            for arena, once in arenas:
                rows = n if once else T * n
                out = torch.empty((rows, *arena.shape[2:]), dtype=arena.dtype, device=dev)
                outs.append(out)
                E = math.prod(arena.shape[2:])
                if out.numel() > 0:
                    fields.append((arena, out, E, arena.size(1), once))
            for j0 in range(0, n, ROLLOUT_MAX_ENVS):
                part_envs = envs[j0:j0 + ROLLOUT_MAX_ENVS]
                for part in _split(fields, ROLLOUT_MAX_FIELDS):
                    lib.rollout_gather([RolloutGatherField(a, o, E, N, n, j0, once)
                                        for a, o, E, N, once in part], part_envs, max(T, 1))
            it = iter(outs)
            observations_batch = {sensor: next(it) for sensor in sensors}
            recurrent_hidden_states_batch = next(it)
            actions_batch = {k: next(it) for k in self.actions}
            prev_actions_batch = {k: next(it) for k in self.actions}
            value_preds_batch, return_batch, masks_batch, old_action_log_probs_batch, adv_targ = it
            yield (observations_batch, recurrent_hidden_states_batch, actions_batch,
                   prev_actions_batch, value_preds_batch, return_batch, masks_batch,
                   old_action_log_probs_batch, adv_targ)
