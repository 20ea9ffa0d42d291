"""What the model files share around their engines: the engine's life cycle on an nn.Module (EngineOwner) and the two halves of
every autograd bridge's backward that do not depend on the model (logit_grads_in, arena_grads)."""
import weakref


class EngineOwner:
    """Mixin of a model whose arithmetic runs in an engine (no parameters, no buffers: state_dict keys and construction order
    are the model's own).  The model sets
      _engine_param   the name of the parameter whose device decides where the engine lives;
      _engine_name    the model's name in the refusal of a CPU model;
      _engine_cls     the engine class, or a static method that returns it (the lazy import of a subclass's engine)."""
    _engine = None
    _engine_name = "r3d_amd.FUTR"

    def _apply(self, fn, *a, **k):
        self._engine = None                     # .to()/.cuda() re-creates parameter storage; re-flatten lazily
        return super()._apply(fn, *a, **k)

    def engine(self):
        dev = self.get_parameter(self._engine_param).device
        if dev.type != "cuda":
            raise RuntimeError(f"{self._engine_name} computes only on an MI355X through libr3d_hip.so; move the model to the "
                               f"GPU with .to('cuda') (there is deliberately no CPU path).")
        if self._engine is None or self._engine.device != dev:
            cls = self._engine_cls
            self._engine = (cls if isinstance(cls, type) else cls())(self, dev)
            ref = weakref.ref(self._engine)
            for p in self.parameters():
                p._r3d_engine = ref              # lets r3d_amd.optim.FlatAdamW find the arena behind its parameters
        return self._engine


def logit_grads_in(w, K, d_act, d_dur, d_seg):
    """The gradients autograd hands a bridge's backward, into the workspace's own buffers: d_act into w.d_actdur[:, :K],
    d_dur into w.d_actdur[:, K], d_seg into w.d_seg (the workspace of a model without a 'seg' output has none).  An output
    the caller's loss did not use arrives as None: its slice is zeroed, not left stale."""
    for dst, src in ((w.d_actdur[:, :K], d_act), (w.d_actdur[:, K], d_dur), (getattr(w, "d_seg", None), d_seg)):
        if dst is None:
            continue
        if src is None:
            dst.zero_()
        else:
            dst.copy_(src.reshape(dst.shape))


def arena_grads(eng, names):
    """A bridge's return for its parameter inputs: copies of the arena gradients, None for the parameters the reference
    leaves without one."""
    return tuple(eng.arena.g(n).clone() if eng.arena.is_live(n) else None for n in names)
