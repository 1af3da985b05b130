"""`OptimState`: the optimizer's state and its step over one parameter set -- the step counter, the last rate, the slot buckets
under the names a checkpoint gives them (`m`, `v`, `velocity`, `ema`), the clip pair, the decay tables and the EMA backup.
`Engine._alloc_params` creates one next to the parameter dict P (`P["opt"]`, `engine.opt`, and `_optim` on the model that holds
P), so every engine of a model shares it as it shares P.  The engine delegates its updates here; `optimizers` reaches it through
the model and imports neither module.  Everything is queued on the context of the parameter bucket.
"""
import ctypes as C
import math

import numpy as np

from . import optimizers as O

SLOTS = ("m", "v", "velocity", "ema")


class OptimState:
    def __init__(self, P, model):
        self.P, self.model, self.ctx = P, model, P["params"].ctx     # model: the one that holds P, where set_state leaves its dict
        self.step = 0               # updates applied: shared by every engine (batch size) of the model
        self.lr = None              # the rate of the last `step_with` update, for fit's history
        self.averaging = False      # inside optimizers.averaged_weights: the parameter bucket holds the EMA
        self.slots = {}             # name -> bucket of n_tr floats, see `slot`
        self.clip = None            # {norm, factor} of ssdseg_grad_norm; None until an optimizer with global_clipnorm steps
        self.clip_parts = None      # its float64 partials
        self.decay_tables = {}      # (weight_decay, names) -> (run_end, run_decay, nruns) on the device
        self.ema_backup = None      # the raw weights while `averaging`

    def slot(self, name, fill=True):
        """the bucket of slot `name`, allocated on first use: `ema` as a copy of the weights (the average before the first update),
        the others as zeros; fill=False leaves it to a caller that overwrites all of it"""
        if name not in self.slots:
            assert name in SLOTS, name
            n = self.P["n_tr"]
            if not fill:
                self.slots[name] = self.ctx.empty(n)
            elif name == "ema":
                self.slots[name] = self.ctx.empty(n).copy_from(self.P["params"])
            else:
                self.slots[name] = self.ctx.zeros(n)
        return self.slots[name]

    def download(self, name):
        """slot `name` as a flat host array; `ema` before the first update is the weights (Keras initialises it from the variable),
        any other slot that does not exist yet is None"""
        buf = self.slots.get(name, self.P["params"] if name == "ema" else None)
        return None if buf is None else buf.download().reshape(-1)

    def restore(self):
        """state that optimizers.set_state / load_state left on the model: into the step counter and the slots (`ema` included)"""
        pend = self.model.__dict__.pop("_optimizer_state", None)
        if pend is None:
            return
        P, model = self.P, self.model
        self.step = pend["step"]
        names = {id(l): l.name for l in model.layers}
        flat = {}
        for (lid, wname), (which, off, shape) in P["index"].items():
            for name in SLOTS:
                arr = pend["arrays"].get(f"{names[lid]}/{wname}:{name}") if which == "params" else None
                if arr is not None:
                    flat.setdefault(name, np.zeros(P["n_tr"], np.float32))[off:off + arr.size] = arr.reshape(-1)
        for name, host in flat.items():
            self.slot(name, fill=False).upload(host)

    # ------------------------------------------------------------------ the step
    def check_not_averaging(self):
        if self.averaging:
            raise RuntimeError("no training step inside optimizers.averaged_weights: the parameter bucket holds the averaged weights")

    def step_with(self, o, grad_scale=1.0):
        """the update of the compiled optimizer `o` (optimizers.Adam / SGD; None: Adam at `adam`'s defaults).  A schedule is
        evaluated at the number of updates already applied -- `step` before it is incremented -- in float64; the C call rounds it
        to float32.  Clipping and the EMA (optimizers._Optimizer._clip_and_ema) stay on the device: the norm entry leaves its factor
        in `clip`, the *_clipped step reads it through a pointer, and the EMA pass follows the step -- all queued, nothing
        downloaded.  An optimizer that does not clip makes the calls it made before there was clipping."""
        self.check_not_averaging()
        if o is None:
            return self.adam(grad_scale=grad_scale)
        self.restore()                              # before the schedule reads the step counter
        P, ctx, n = self.P, self.ctx, C.c_size_t(self.P["n_tr"])
        lr = self.lr = O.rate_at(o.learning_rate, self.step)
        clip = None
        if o.global_clipnorm is not None:
            if self.clip is None:
                self.clip = ctx.zeros(2)
                self.clip_parts = ctx.empty(max(ctx.lib.ssdseg_grad_norm_parts(P["n_tr"]), 1), np.float64)
            ctx.call("ssdseg_grad_norm", P["grads"], n, grad_scale, o.global_clipnorm, self.clip_parts, self.clip)
            clip = self.clip.view(1, (1,)), math.inf
        elif o.clipvalue is not None:
            clip = None, o.clipvalue
        if o.use_ema:
            self.slot("ema")
        decay = self._decay_table(o)
        if isinstance(o, O.SGD):
            self.step += 1
            velocity = self.slot("velocity") if o.momentum > 0 else None     # allocated on first use: an Adam run never pays for it
            ctx.call("ssdseg_sgd_step" if clip is None else "ssdseg_sgd_step_clipped", P["params"], P["grads"], velocity, n, lr, o.momentum,
                     int(o.nesterov), grad_scale, *(decay or (None, None, 0)), *(clip or ()))
        else:
            self.adam(lr, o.beta_1, o.beta_2, o.epsilon, grad_scale, decay, clip)
        if o.use_ema:
            ctx.call("ssdseg_ema_update", self.slots["ema"], P["params"], n, o.ema_momentum)
            if o.ema_overwrite_frequency and self.step % o.ema_overwrite_frequency == 0:
                P["params"].copy_from(self.slots["ema"])

    def _decay_table(self, o):
        """the optimizer's weight-decay run table over the parameter bucket (optimizers.decay_runs; None without decay): built once
        per (weight_decay, names) from P["index"] in bucket order, uploaded once"""
        if o.weight_decay == 0.0:
            return None
        key = (o.weight_decay, o.weight_decay_names)
        if key not in self.decay_tables:
            entries = sorted((off, wname, int(np.prod(shape))) for (_, wname), (which, off, shape) in self.P["index"].items() if which == "params")
            ends, lams = O.decay_runs([(wname, off, size) for off, wname, size in entries], *key)
            assert ends.size and ends[-1] == self.P["n_tr"]
            self.decay_tables[key] = (self.ctx.array(ends), self.ctx.array(lams), int(ends.size))
        return self.decay_tables[key]

    def adam(self, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0, decay=None, clip=None):
        """one Adam update from bare hyper-parameters: the legacy entry without a table or a clip, which the benchmark times"""
        self.restore()
        P = self.P
        self.step += 1
        args = (P["params"], P["grads"], self.slots.get("m"), self.slots.get("v"), C.c_size_t(P["n_tr"]), lr, beta1, beta2, eps, self.step, grad_scale)
        if clip is not None:
            self.ctx.call("ssdseg_adamw_step_clipped", *args, *(decay or (None, None, 0)), *clip)
        elif decay is None:
            self.ctx.call("ssdseg_adam_step", *args)
        else:
            self.ctx.call("ssdseg_adamw_step", *args, *decay)

    # ------------------------------------------------------------------ the averaged weights
    def finalize(self):
        """the weights become the averaged weights, for good (no EMA bucket yet: they are the average already)"""
        if "ema" in self.slots:
            if self.averaging:
                raise RuntimeError("inside averaged_weights the weights are the average already")
            self.P["params"].copy_from(self.slots["ema"])

    def swap_in_average(self) -> bool:
        """the parameter bucket takes the EMA, the raw weights wait in the backup bucket (allocated on first use); False, and nothing
        done, where no update has been made yet: the weights are the average"""
        if "ema" not in self.slots:
            return False
        if self.averaging:
            raise RuntimeError("averaged_weights blocks do not nest")
        if self.ema_backup is None:
            self.ema_backup = self.ctx.empty(self.P["n_tr"])
        self.ema_backup.copy_from(self.P["params"])
        self.P["params"].copy_from(self.slots["ema"])
        self.averaging = True
        return True

    def swap_out_average(self):
        self.P["params"].copy_from(self.ema_backup)
        self.averaging = False
