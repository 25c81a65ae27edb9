"""`fit`: the thin training loop that the reference gets from its Lightning shell (train_generative_sensing_model.py) — host
code only.  Learning rate from the base rate, `training_step` per batch, periodic validation, checkpoints that
`VQModel(ckpt_path=...)` reads, and resumption (weights, Adam moments, step count, loader position and RNG).  Both phases: the
pair batches of `conditional_generation` and the single-frame `image` batches of `codebook` (whose loaders carry no RNG: their
position alone resumes them).  Not here: LR schedulers, image logging, wandb, signal handlers, distributed samplers."""
import os

import torch


def _world_size():
    import torch.distributed as dist
    return dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1


def _dataset_name(model):
    dc = model.data_config
    return dc["dataset"] if isinstance(dc, dict) else dc.dataset


def _optimizer_states(model, tr):
    """{"ae" | "disc": {parameter name: (exp_avg, exp_avg_sq)}} on the CPU"""
    names = {p: n for n, p in model.named_parameters()}
    out = {"ae": {names[p]: (m.cpu(), v.cpu()) for p, (m, v) in tr.state.items()}}
    if hasattr(tr, "dstate"):
        out["disc"] = {names[p]: (m.cpu(), v.cpu()) for p, (m, v) in tr.dstate.items()}
    return out


def _restore_optimizer_states(model, tr, states):
    params = dict(model.named_parameters())
    for key, state in (("ae", tr.state), ("disc", getattr(tr, "dstate", None))):
        for n, (m, v) in states.get(key, {}).items():
            p = params[n]
            state[p] = (m.to(p.device).clone(), v.to(p.device).clone())


def save_checkpoint(path, model, tr, loader):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save({"state_dict": {k: v.cpu() for k, v in model.state_dict().items()}, "global_step": int(tr.global_step),
                "optimizer_states": _optimizer_states(model, tr), "loader_state": loader.state_dict()}, path)
    return path


def _validate(model, tr, loader, val_batches):
    tr.validation_epoch_start()
    for i, batch in enumerate(loader):
        if val_batches is not None and i >= val_batches:
            break
        if model.phase == "conditional_generation":
            x, x_dst, mask, _ = model.get_x(batch, _dataset_name(model), return_extrapolation_mask=True)
        else:
            x = model.get_input(model.image_key, batch).to(model.device)
            x_dst, mask = x, None
        tr.validation_step(x, x_dst, mask)
    return tr.validation_epoch_end()


def fit(model, datamodule, max_steps, val_every=None, val_batches=None, ckpt_dir=None, ckpt_every=None, resume=None, log=None,
        base_learning_rate=None):
    """Train `model` (a VQModel on the GPU, with a `lossconfig`) on `datamodule.train_dataloader()` until `global_step`
    reaches `max_steps`.

    learning rate = world size * batch size * base rate (`base_learning_rate`, default: the model's `learning_rate`, which
    is the shipped configs' base rate).  `log(step, dict)` receives `model.logged` after every step and the validation epoch
    means every `val_every` steps (`val_batches` batches of `val_dataloader()`, all if None).  Every `ckpt_every` steps
    `ckpt_dir/step_<n>.ckpt` and `ckpt_dir/last.ckpt` are written: {"state_dict", "global_step", "optimizer_states",
    "loader_state"}.  `resume=path` continues such a checkpoint: the run is then the one an uninterrupted call would have
    made (the online k-means refresh state is not part of a checkpoint).  Returns {"global_step", "checkpoints"}."""
    base = float(base_learning_rate if base_learning_rate is not None else type(model).learning_rate)
    model.learning_rate = _world_size() * datamodule.batch_size * base
    if resume is not None:
        ckpt = torch.load(resume, map_location="cpu")
        model.init_loss()                    # the checkpoint's `loss.*` tensors (PatchGAN weights, BatchNorm statistics) have a home
        model.load_state_dict(ckpt["state_dict"], strict=False)
    tr = model._trainer_for_step()
    tr.lr = float(model.learning_rate)
    loader = datamodule.train_dataloader()
    if resume is not None:
        from . import training
        training._invalidate_packs(model)
        _restore_optimizer_states(model, tr, ckpt["optimizer_states"])
        tr.global_step = model.global_step = int(ckpt["global_step"])
        loader.load_state_dict(ckpt["loader_state"])
    if len(loader) == 0:
        raise ValueError("fit: the training loader has no batch (dataset smaller than one batch with drop_last?)")
    written = []
    it = iter(loader)
    try:
        while tr.global_step < max_steps:
            try:
                batch = next(it)
            except StopIteration:
                it = iter(loader)
                continue
            model.training_step(batch, tr.global_step)
            step = int(tr.global_step)
            if log is not None:
                log(step, dict(model.logged))
            if val_every and step % val_every == 0:
                val_loader = datamodule.val_dataloader()
                try:
                    out = _validate(model, tr, val_loader, val_batches)
                finally:
                    val_loader.close()
                if log is not None:
                    log(step, out)
            if ckpt_dir is not None and ckpt_every and step % ckpt_every == 0:
                written.append(save_checkpoint(os.path.join(ckpt_dir, f"step_{step:07d}.ckpt"), model, tr, loader))
                save_checkpoint(os.path.join(ckpt_dir, "last.ckpt"), model, tr, loader)
    finally:
        loader.close()
    return {"global_step": int(tr.global_step), "checkpoints": written}
