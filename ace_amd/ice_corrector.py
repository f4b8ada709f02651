"""Post-step sea-ice corrector: fme/core/corrector/ice.py (``IceCorrectorConfig``, registered as "ice_corrector").

Mirror of the reference's configuration (same fields and defaults, so a checkpoint's step config round-trips) and of the one
correction it builds, ``IceBudgetCorrectionConfig``: for each corrected variable - ice mass, ice concentration, snow mass, in
that order - the three predicted budget terms (source, sink, transport) are rebalanced so that the mass they imply,
``old + dt * (source + sink + transport)``, is not negative, not above 1 (a concentration) and zero where there is no ice, and
the prognostic variable is rebuilt from them.

Two paths compute the same bits.  On the CPU (and whenever ``IceCorrector.fused`` is False) the correction runs as the readable
torch restatement below, pinned to the reference by tests/golden/gen_ice_corrector_*.pt.  With the fields on the GPU it is
``ace_ice_budget_apply`` (include/ace_sfno.h, ace_amd/csrc/ice_budget.hip): two launches per variable and not one host readback,
where the reference's ``if torch.any(mask)`` reads the device up to three times per variable.  The fused path corrects the output
tensors in place; the input is only read.  The torch path, like the reference, returns new tensors for the fields it changes."""
import ctypes
import dataclasses
import functools
from ctypes import c_long
from typing import Any, Dict, List, Mapping, Optional, Tuple

import torch

from ._lib import check

TensorMapping = Mapping[str, torch.Tensor]
TensorDict = Dict[str, torch.Tensor]

SIC_NAMES = ("siconc", "sea_ice_fraction", "ocean_sea_ice_fraction")      # ice.py:155: capped at 1 (area_mode)
ICE_MASS_NAME, SNOW_MASS_NAME = "simass", "sisnmass"


# ---------------------------------------------------------------------------------------------------------------------
# the correction (ice.py:31-198)
def _rebalance(s, k, t, mask, mass, sign):
    """ice.py:69-106: spread ``mass`` over the non-zero terms of the pixels in ``mask`` (all of it onto the transport where all
    three are zero); everywhere, masked or not, a sink that ends positive and a source that ends negative move to the transport."""
    dtype = mass.dtype
    zero = torch.zeros_like(mass)
    nz_s, nz_k, nz_t = s.abs() > 0, k.abs() > 0, t.abs() > 0
    n_active = nz_s.to(dtype) + nz_k.to(dtype) + nz_t.to(dtype)
    share = torch.where(mask & (n_active > 0), mass / n_active.clamp(min=1), zero)
    resid_s = torch.where(mask & nz_s, share, zero)
    resid_k = torch.where(mask & nz_k, share, zero)
    resid_t = torch.where(mask & nz_t, share, zero)
    resid_t = torch.where(mask & (n_active == 0), mass, resid_t)
    tmp = k + sign * resid_k
    k_overshoot = torch.where(tmp > 0, tmp, zero)
    resid_k = resid_k - k_overshoot
    resid_t = resid_t + k_overshoot
    tmp = s + sign * resid_s
    s_overshoot = torch.where(tmp < 0, tmp, zero)
    resid_s = resid_s - sign * s_overshoot
    resid_t = resid_t + sign * s_overshoot
    return s + sign * resid_s, k + sign * resid_k, t + sign * resid_t


def constrain_budgets(old_mass, source, sink, transport, timestep: float, area_mode: bool = False, ice_mask=None):
    """ice.py:31-134 on fp64 tensors.  Each stage runs for the whole tensor if its mask holds anywhere, and not at all
    otherwise (``torch.any``: a host readback - the fused path carries these flags on the device)."""
    s, k, t = source * timestep, sink * timestep, transport * timestep
    zero = torch.zeros_like(old_mass)
    new_mass = old_mass + (s + k + t)
    neg_mask = new_mass < 0
    if torch.any(neg_mask):
        s, k, t = _rebalance(s, k, t, neg_mask, torch.where(neg_mask, -new_mass, zero), 1)
    if area_mode:
        new_mass = old_mass + (s + k + t)
        high_mask = new_mass > 1
        if torch.any(high_mask):
            s, k, t = _rebalance(s, k, t, high_mask, torch.where(high_mask, new_mass - 1, zero), -1)
    if ice_mask is not None:
        new_mass = old_mass + (s + k + t)
        high_mask = (ice_mask == 0) & (new_mass > 0)
        if torch.any(high_mask):
            s, k, t = _rebalance(s, k, t, high_mask, torch.where(high_mask, new_mass, zero), -1)
    # a tensor divisor: torch turns a division by a Python scalar into a multiplication by its reciprocal on the GPU, which is
    # not the reference's (CPU) quotient in the last bit
    dt = torch.as_tensor(timestep, dtype=old_mass.dtype, device=old_mass.device)
    return s / dt, k / dt, t / dt


# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class IceBudgetCorrectionConfig:
    """{'variable': ['source_term', 'sink_term', 'transport_term']}, e.g. {'siconc': ['LSRCc', 'LSNKc', 'XPRTc']}."""
    corrected_variables: Optional[Dict[str, List[str]]] = None

    def plan(self) -> List[Tuple[str, Tuple[str, str, str], bool, bool]]:
        """(variable, its three terms, area_mode, masked) in processing order (ice.py:155-177): ice mass, the concentration,
        snow mass; every variable but the first is masked by the corrected mass of the first.  Other keys are ignored."""
        cv = self.corrected_variables
        if cv is None:
            return []
        sic = [n for n in SIC_NAMES if n in cv]
        if len(sic) > 1:
            raise NotImplementedError(
                f"ice budget correction of more than one concentration variable ({sic}): the reference iterates a Python set "
                "of these names, so their order, and which of them masks the others, changes with the process's hash seed")
        order = ([ICE_MASS_NAME] if ICE_MASS_NAME in cv else []) + sic + ([SNOW_MASS_NAME] if SNOW_MASS_NAME in cv else [])
        out = []
        for i, name in enumerate(order):
            terms = tuple(cv[name])
            if len(terms) != 3:
                raise ValueError(f"corrected_variables['{name}'] must name three terms (source, sink, transport), got {list(terms)}")
            out.append((name, terms, name in SIC_NAMES, i > 0))
        return out


@dataclasses.dataclass
class IceCorrectorConfig:
    budget_correction: Optional[IceBudgetCorrectionConfig] = None
    # CorrectorConfigABC (registry.py:14-62): a training-epoch schedule; inference always applies the corrector
    corrector_disabled_epochs: int = 0

    def __post_init__(self):
        from .ocean_corrector import _sub
        if self.corrector_disabled_epochs < 0:
            raise ValueError(f"corrector_disabled_epochs must be non-negative, got {self.corrector_disabled_epochs}")
        self.budget_correction = _sub(IceBudgetCorrectionConfig, self.budget_correction)
        if self.budget_correction is not None:
            self.budget_correction.plan()      # the refusals, at build time

    @classmethod
    def from_state(cls, state: Mapping[str, Any]) -> "IceCorrectorConfig":
        state = dict(state)
        if "type" in state and "config" in state:      # CorrectorSelector form (fme/core/registry/corrector.py)
            if set(state) - {"type", "config", "corrector_disabled_epochs"}:
                raise ValueError(f"unknown corrector selector fields: {sorted(state)}")
            if state.get("corrector_disabled_epochs", 0) != 0:
                raise ValueError("corrector_disabled_epochs must be set on the wrapped corrector config (inside "
                                 "`config:`), not on the CorrectorSelector.")
            if state["type"] != "ice_corrector":
                raise ValueError(f"not an ice corrector: {state['type']!r}")
            state = dict(state["config"] or {})
        unknown = set(state) - {f.name for f in dataclasses.fields(cls)}
        if unknown:
            raise ValueError(f"unknown ice corrector fields: {sorted(unknown)}")
        return cls(**state)

    def unsupported(self, dataset_info=None) -> List[str]:
        """the budget correction needs no geometry: nothing a dataset_info can lack"""
        return []

    def get_corrector(self, dataset_info=None, ignore_unsupported: bool = False) -> Optional["IceCorrector"]:
        corrector = IceCorrector(self, dataset_info)
        return corrector if corrector.corrections else None


class IceCorrector:
    """CorrectionSequence built as in ice.py:246-256; the same call signature and return as the other correctors:
    ``(input, gen, forcing, state) -> (corrected gen dict, state)`` (the ice corrector carries no state)."""

    def __init__(self, config: IceCorrectorConfig, dataset_info=None):
        self._cfg = config
        bc = config.budget_correction
        self._plan = bc.plan() if bc is not None else []
        self.corrections: List[str] = ["budget_correction"] if self._plan else []
        ts = getattr(dataset_info, "timestep", None)
        self._dt = ts.total_seconds() if ts is not None else None
        if self._plan and self._dt is None:
            raise ValueError("the ice budget correction needs the dataset's timestep")
        self.force_positive_names: List[str] = []
        self.fused = True              # GPU tensors take the HIP path; False: the torch ops on any device
        self._handles: Dict[Any, "FusedIceCorrector"] = {}

    @property
    def config(self) -> IceCorrectorConfig:
        return self._cfg

    @property
    def plan(self):
        return list(self._plan)

    @property
    def timestep_seconds(self) -> Optional[float]:
        return self._dt

    def __call__(self, input_data: TensorMapping, gen_data: TensorMapping, forcing_data: TensorMapping,
                 corrector_state=None) -> Tuple[TensorDict, Any]:
        gen = dict(gen_data)
        if not self.corrections:
            return gen, corrector_state
        dev = next(iter(gen.values())).device
        if self.fused and dev.type == "cuda":
            return self._fused(input_data, gen, forcing_data), corrector_state
        return self.torch_apply(input_data, gen, forcing_data), corrector_state

    def torch_apply(self, input_data: TensorMapping, gen_data: TensorMapping, forcing_data: TensorMapping = None) -> TensorDict:
        """ice.py:136-198: fp64 working copies (a later variable's mask reads the fp64 mass an earlier one wrote, and a term two
        variables share is read as the earlier one left it), fp32 results; uncorrected fields pass through."""
        gen = dict(gen_data)
        work: Dict[str, torch.Tensor] = {}
        get = lambda name: work[name] if name in work else gen_data[name].double()
        mask_var = self._plan[0][0] if self._plan else None
        for name, terms, area_mode, masked in self._plan:
            old = input_data[name].double()
            budgets = constrain_budgets(old, get(terms[0]), get(terms[1]), get(terms[2]), self._dt, area_mode=area_mode,
                                        ice_mask=work[mask_var] if masked else None)
            for term, b in zip(terms, budgets):
                work[term] = b
            work[name] = old + self._dt * (budgets[0] + budgets[1] + budgets[2])
        gen.update({k: v.float() for k, v in work.items()})
        return gen

    # ---- the HIP path ------------------------------------------------------------------------------------------------
    def handle(self, batch: int, img_shape: Tuple[int, int], device) -> "FusedIceCorrector":
        key = (str(torch.device(device)), batch, *img_shape)
        h = self._handles.get(key)
        if h is None:
            h = self._handles[key] = FusedIceCorrector(self, batch, img_shape, device)
        return h

    def _fused(self, input_data: TensorMapping, gen: TensorDict, forcing_data: TensorMapping) -> TensorDict:
        any_t = gen[self._plan[0][0]] if self._plan[0][0] in gen else next(iter(gen.values()))
        return self.handle(any_t.shape[0], (any_t.shape[-2], any_t.shape[-1]), any_t.device)(input_data, gen, forcing_data)

    def launches(self) -> Tuple[int, int]:
        """(flags, apply) launches made by the HIP path of this corrector so far, over all its handles (the route query)."""
        return (sum(h.launched[0] for h in self._handles.values()), sum(h.launched[1] for h in self._handles.values()))


# ---------------------------------------------------------------------------------------------------------------------
_check = functools.partial(check, family="ice_budget")


class FusedIceCorrector:
    """One handle per (device, batch, grid) of an ``IceCorrector``: it owns the flag and mask scratch, resolves the corrected
    variables to ``{pointer, per-sample stride}`` planes of the caller's tensors (``fields``) and launches on a stream
    (``apply``).  Output planes are corrected in place; a strided view of a larger tensor is used as it is."""

    def __init__(self, corrector: IceCorrector, batch: int, img_shape: Tuple[int, int], device):
        from . import _lib
        H, W = img_shape
        self.batch, self.shape, self.device = batch, (H, W), torch.device(device)
        self._corrector = corrector
        self._plan = corrector.plan
        if len(self._plan) > _lib.ICE_MAX_VARS:
            raise NotImplementedError(f"the fused ice corrector corrects up to {_lib.ICE_MAX_VARS} variables")
        written = [n for name, terms, _, _ in self._plan for n in (*terms, name)]
        if len(set(written)) != len(written):
            # the reference hands a shared term from one variable to the next in fp64; the planes hold it rounded to fp32
            raise NotImplementedError("fused ice corrector: a field is written by two corrected variables "
                                      f"({sorted(n for n in set(written) if written.count(n) > 1)}); use the torch path "
                                      "(IceCorrector.fused = False)")
        self._dt = float(corrector.timestep_seconds)
        self.launched = [0, 0]
        self.scratch = self._make_scratch(_lib.lib().ace_ice_budget_scratch_bytes(batch, H * W))

    def _make_scratch(self, nbytes: int) -> torch.Tensor:
        return torch.zeros(nbytes, dtype=torch.uint8, device=self.device)

    def fields(self, inp, gen, forcing=None):
        """The planes of one step: a missing field raises KeyError, as the reference does."""
        from . import _lib
        f = _lib.IceFields()
        plane = lambda dst, t, name: _lib.bind_plane(dst, t, self.batch, self.shape, self.device, "fused ice corrector", name)
        for i, (name, terms, area_mode, masked) in enumerate(self._plan):
            v = f.var[i]
            plane(v.old_mass, inp[name], name)
            for attr, term in zip(("source", "sink", "transport"), terms):
                plane(getattr(v, attr), gen[term], term)
            plane(v.mass, gen[name], name)
            v.area_mode, v.masked = int(area_mode), int(masked)
        f.nvars = len(self._plan)
        return f

    def __call__(self, inp, gen, forcing=None):
        missing = [name for name, _, _, _ in self._plan if name not in gen]
        if missing:      # the reference adds a corrected variable the network does not predict; in place needs somewhere to write
            gen.update({n: torch.empty_like(inp[n]) for n in missing})
        f = self.fields(inp, gen, forcing)
        with torch.cuda.device(self.device):
            self.apply(f, torch.cuda.current_stream(self.device).cuda_stream)
        return gen

    def apply(self, fields, stream: int) -> None:
        """One step on planes resolved once by ``fields`` (static buffers: ``OceanRolloutEngine`` keeps a struct per step)."""
        from . import _lib
        B, (H, W) = self.batch, self.shape
        _check(_lib.lib().ace_ice_budget_apply(ctypes.byref(fields), self._dt, B, H, W, self.scratch.data_ptr(), stream))
        self.launched[0] += fields.nvars
        self.launched[1] += fields.nvars

    def launches(self) -> Tuple[int, int]:
        return tuple(self.launched)


def library_launches() -> Tuple[int, int, int]:
    """(flags passes, apply passes, flag clearings) the library has enqueued in this process (``ace_ice_budget_launches``)."""
    from . import _lib
    a, b, c = c_long(0), c_long(0), c_long(0)
    _check(_lib.lib().ace_ice_budget_launches(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return a.value, b.value, c.value
