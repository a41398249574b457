"""DAgger / recollect inner step: restatement of
BaseVLNCETrainer._update_agent (vlnce_baselines/common/base_il_trainer.py:134-180)
for callers that run without habitat (bench.py, tests).  The real trainers call
the policy's build_distribution() themselves and need nothing from here."""
import torch
import torch.nn.functional as F

from .aux_losses import AuxLosses


class ILLossFn(torch.autograd.Function):
    """The imitation-learning objective (base_il_trainer.py:159-172: inflection-weighted cross
    entropy normalised per episode, plus the auxiliary term, over the accumulation scalar) as ONE
    launch that also produces the logits gradient (vlnce_il_loss), instead of the chain of small
    elementwise / reduction launches forward and as many backward, all host-paced.
    forward(logits [T, N, A], targets [T, N] int64, weights [T, N], aux: device scalar | None,
    inv_scalar) -> (loss [], stats [3] = loss, action_loss, aux)."""

    @staticmethod
    def forward(ctx, logits, targets, weights, aux, inv_scalar):
        from . import ops

        T, N, A = logits.shape
        stats = torch.empty(3, device=logits.device, dtype=torch.float32)
        dlogits = torch.empty((T * N, A), device=logits.device, dtype=torch.float32)
        ops.L().il_loss(ops._f32c(logits.detach()), targets.contiguous(),
                        ops._f32c(weights.detach()),
                        None if aux is None else ops._f32c(aux.detach()).reshape(1), inv_scalar,
                        T, N, A, stats, dlogits)
        ctx.save_for_backward(dlogits)
        ctx.shape, ctx.inv_scalar = logits.shape, inv_scalar
        ctx.aux_shape = None if aux is None else aux.shape
        loss = stats[0].clone()
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, g_loss, _g_stats):
        (dlogits,) = ctx.saved_tensors
        g_aux = None
        if ctx.aux_shape is not None and ctx.needs_input_grad[3]:
            g_aux = (g_loss * ctx.inv_scalar).reshape(ctx.aux_shape)
        return (dlogits * g_loss).view(ctx.shape), None, None, g_aux, None


def il_loss_supported(logits_TNA):
    from . import ops

    return bool(ops.L().il_loss_supported(*logits_TNA.shape))


def il_loss(logits_TNA, corrected_actions, weights, aux=0.0, loss_accumulation_scalar=1):
    """(loss, stats) of one `_update_agent` minibatch in one launch (ILLossFn); stats [3] =
    {loss, action_loss, aux_loss} on the device, non-differentiable.  `aux` is what
    AuxLosses.reduce returned: a scalar tensor (gradient flows into it) or a Python number."""
    if not isinstance(aux, torch.Tensor):
        aux = None if aux == 0 else torch.tensor(float(aux), device=logits_TNA.device)
    return ILLossFn.apply(logits_TNA, corrected_actions, weights, aux,
                          1.0 / loss_accumulation_scalar)


def update_agent(policy, optimizer, observations, prev_actions, not_done_masks,
                 corrected_actions, weights, hidden_size, step_grad=True,
                 loss_accumulation_scalar=1, grad_hook=None, fused_loss=False):
    """fused_loss=True: the objective and its gradient are one launch (il_loss), the progress
    monitor's term one more (AuxLosses.fused), and the three floats one read-back.  A batch the
    kernel does not take (il_loss_supported) goes the default way."""
    T, N = corrected_actions.size()
    recurrent_hidden_states = torch.zeros(
        N, policy.net.num_recurrent_layers, hidden_size, device=corrected_actions.device)
    AuxLosses.clear()

    def reduce_aux():
        return AuxLosses.reduce((weights > 0).view(-1)) if AuxLosses.is_active() else 0.0

    if fused_loss:
        with AuxLosses.fused():
            distribution = policy.build_distribution(
                observations, recurrent_hidden_states, prev_actions, not_done_masks)
            aux_loss = reduce_aux()
        logits = distribution.logits.view(T, N, -1)
        fused_loss = il_loss_supported(logits)
    else:
        distribution = policy.build_distribution(
            observations, recurrent_hidden_states, prev_actions, not_done_masks)
        logits = distribution.logits.view(T, N, -1)
        aux_loss = None
    if fused_loss:
        loss, stats = il_loss(logits, corrected_actions, weights, aux_loss, loss_accumulation_scalar)
    else:
        action_loss = F.cross_entropy(logits.permute(0, 2, 1), corrected_actions, reduction="none")
        action_loss = ((weights * action_loss).sum(0) / weights.sum(0)).mean()
        if aux_loss is None:
            aux_loss = reduce_aux()
        loss = (action_loss + aux_loss) / loss_accumulation_scalar
    loss.backward()
    if grad_hook is not None:
        grad_hook()  # data-parallel gradient all-reduce (vlnce_amd.distributed)
    if step_grad:
        optimizer.step()
        optimizer.zero_grad()
    if fused_loss:
        loss, action_loss, aux = stats.tolist()   # one read-back for the three floats
        return loss, action_loss, aux if isinstance(aux_loss, torch.Tensor) else 0.0
    # the reference ends every step with three host read-backs (base_il_trainer.py:176-180):
    # `loss.item(), action_loss.item(), aux_loss.item()` -- Python floats, one sync each; the timed
    # loop of bench.py consumes them exactly as the trainers' loggers do
    if isinstance(aux_loss, torch.Tensor):
        aux_loss = aux_loss.item()
    return loss.item(), action_loss.item(), aux_loss
