"""Single-module step (fme/core/step/single_module.py:48-511, 595-733; args.py:8-56; output.py:12-28).

normalize -> pack (in_names order) -> network -> unpack (out_names order) -> denormalize
[-> residual add] [-> prescribed prognostic overwrite].  The corrector and ocean hooks
of the reference default to identity / None and are not carried;
configuring them raises instead of being silently ignored."""

import dataclasses
from collections.abc import Callable, Mapping
from typing import Any, Dict, List, Optional

import torch
from torch import nn

from .normalizer import StandardNormalizer
from .packer import Packer
from .registry import ModuleSelector

TensorMapping = Mapping[str, torch.Tensor]
TensorDict = Dict[str, torch.Tensor]


@dataclasses.dataclass
class NormalizationConfig:
    """means/stds per variable name (fme/core/normalizer.py NormalizationConfig with explicit dicts)."""

    means: Mapping[str, float]
    stds: Mapping[str, float]
    fill_nans_on_normalize: bool = False
    fill_nans_on_denormalize: bool = False

    def build(self, names: List[str], device=None) -> StandardNormalizer:
        means = {k: torch.tensor(self.means[k], dtype=torch.float) for k in names}
        stds = {k: torch.tensor(self.stds[k], dtype=torch.float) for k in names}
        return StandardNormalizer(means, stds, self.fill_nans_on_normalize, self.fill_nans_on_denormalize, device=device)


class StepArgs:
    """args.py:8-56."""

    def __init__(self, input: TensorMapping, next_step_input_data: TensorMapping, labels=None,
                 data_mask: Optional[TensorMapping] = None, stepper_state=None):
        self.input = input
        self.next_step_input_data = next_step_input_data
        self.labels = labels
        self.data_mask = data_mask
        self.stepper_state = stepper_state

    def apply_input_process_func(self, func: Callable[[TensorMapping], TensorMapping]) -> "StepArgs":
        return StepArgs(input=func(self.input), next_step_input_data=func(self.next_step_input_data),
                        labels=self.labels, data_mask=self.data_mask, stepper_state=self.stepper_state)


@dataclasses.dataclass
class StepperState:
    """fme/core/stepper_state.py:22-127: the state threaded from one step to the next and from one ``predict`` call to the
    next - the corrector's per-sample state and the seedable random source of stochastic modules (``ace_amd.rand.RandomState``;
    None: the global torch RNG).  The stepper does not look inside either."""
    corrector_state: Any = None
    random_state: Any = None

    def to_state_dict(self) -> Dict[str, torch.Tensor]:
        """stepper_state.py:87-107: present sub-states, keys namespaced, a ``<name>.present`` marker each (restart files)"""
        out: Dict[str, torch.Tensor] = {}
        if self.corrector_state is not None:
            out["corrector_state.present"] = torch.tensor(True)
            mass = getattr(self.corrector_state, "global_dry_air_mass", None)
            if mass is not None:
                out["corrector_state.global_dry_air_mass"] = mass
        if self.random_state is not None:
            out["random_state.present"] = torch.tensor(True)
            for k, v in self.random_state.to_state_dict().items():
                out[f"random_state.{k}"] = v
        return out

    @classmethod
    def from_state_dict(cls, state: Mapping[str, torch.Tensor]) -> "StepperState":
        """stepper_state.py:109-124: a sub-state without its marker comes back as None"""
        from .corrector import CorrectorState
        from .rand import RandomState
        cs = rs = None
        if "corrector_state.present" in state:
            cs = CorrectorState(global_dry_air_mass=state.get("corrector_state.global_dry_air_mass"))
        if "random_state.present" in state:
            rs = RandomState.from_state_dict({"generator_state": state["random_state.generator_state"]})
        return cls(corrector_state=cs, random_state=rs)


@dataclasses.dataclass
class StepOutput:
    """output.py:12-28.  ``corrector_diagnostics``: name -> ``corrected - network output`` of the names the corrector wrote, filled
    only when the step is asked for it (``step_diagnostics=True``); empty otherwise."""

    output: TensorDict
    stepper_state: Any = None
    corrector_diagnostics: Dict[str, torch.Tensor] = dataclasses.field(default_factory=dict)


@dataclasses.dataclass
class SecondaryDecoderConfig:
    """fme/core/step/secondary_decoder.py:16-42: additional diagnostics computed column-locally from the network's (normalised)
    output tensor by a second registry network (normally the "MLP")."""
    secondary_diagnostic_names: List[str]
    network: Any

    def __post_init__(self):
        self.secondary_diagnostic_names = list(self.secondary_diagnostic_names)
        if isinstance(self.network, Mapping):
            self.network = ModuleSelector(**{k: (dict(v) if k == "config" else v) for k, v in self.network.items()})

    @classmethod
    def from_state(cls, state) -> Optional["SecondaryDecoderConfig"]:
        if state is None or isinstance(state, cls):
            return state
        extra = set(state) - {"secondary_diagnostic_names", "network"}
        if extra:
            raise ValueError(f'can not match {sorted(extra)} to any data class field of "SecondaryDecoderConfig"')
        return cls(**state)

    def build(self, n_in_channels: int, dataset_info) -> "SecondaryDecoder":
        return SecondaryDecoder(n_in_channels, self.secondary_diagnostic_names, self.network, dataset_info)


class SecondaryDecoder:
    """secondary_decoder.py:45-112."""
    CHANNEL_DIM = -3

    def __init__(self, in_dim: int, out_names: List[str], network: ModuleSelector, dataset_info):
        self._module = network.build(n_in_channels=in_dim, n_out_channels=len(out_names), dataset_info=dataset_info)
        self._packer = Packer(list(out_names))

    @property
    def torch_modules(self) -> nn.ModuleList:
        return nn.ModuleList([self._module.torch_module])

    def to(self, device) -> "SecondaryDecoder":
        self._module = self._module.to(device)
        return self

    def wrap_module(self, wrapper) -> "SecondaryDecoder":
        self._module = self._module.wrap_module(wrapper)
        return self

    def __call__(self, x: torch.Tensor) -> TensorDict:
        return self._packer.unpack(self._module(x), axis=self.CHANNEL_DIM)

    def get_module_state(self) -> dict:
        return self._module.get_state()

    def load_module_state(self, state: dict) -> None:
        state = dict(state)
        if state and all(k.startswith("module.") or k == "label_encoding" for k in state):      # DummyWrapper / DDP prefix
            state = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}
        self._module.load_state(state)


@dataclasses.dataclass
class SingleModuleStepConfig:
    """single_module.py:48-259, restricted to the options on the hot path."""

    builder: ModuleSelector
    in_names: List[str]
    out_names: List[str]
    normalization: NormalizationConfig
    secondary_decoder: Any = None
    ocean: Any = None
    corrector: Any = None
    next_step_forcing_names: List[str] = dataclasses.field(default_factory=list)
    prescribed_prognostic_names: List[str] = dataclasses.field(default_factory=list)
    residual_prediction: bool = False
    include_channel_mask_inputs: bool = False
    global_mean_removal: Any = None
    input_dropout: Any = None

    def __post_init__(self):
        from .corrector import AtmosphereCorrectorConfig
        from .ocean import OceanConfig
        from .ice_corrector import IceCorrectorConfig
        from .ocean_corrector import OceanCorrectorConfig, corrector_config_from_state
        from .global_mean_removal import config_from_state as gmr_config_from_state
        if self.input_dropout is not None:
            raise NotImplementedError("SingleModuleStepConfig.input_dropout is outside the accelerated hot path")
        # a configuration instance or its state (as found in a checkpoint's step config); validated as the reference does
        # (single_module.py:101-102)
        self.global_mean_removal = gmr_config_from_state(self.global_mean_removal)
        if self.global_mean_removal is not None:
            self.global_mean_removal.validate_names(self.in_names, self.out_names)
        self.secondary_decoder = SecondaryDecoderConfig.from_state(self.secondary_decoder)
        # ocean / corrector: dataclass instances or their state dicts (as found in a checkpoint's step config)
        if isinstance(self.ocean, dict):
            self.ocean = OceanConfig.from_state(self.ocean)
        if self.ocean is not None and not isinstance(self.ocean, OceanConfig):
            raise NotImplementedError("SingleModuleStepConfig.ocean must be an OceanConfig (prescribed SST or slab ocean) or its state")
        if not isinstance(self.corrector, (AtmosphereCorrectorConfig, OceanCorrectorConfig, IceCorrectorConfig, dict, type(None))):
            raise NotImplementedError("SingleModuleStepConfig.corrector must be an AtmosphereCorrectorConfig, an "
                                      "OceanCorrectorConfig, an IceCorrectorConfig or its state")
        if self.corrector is None or isinstance(self.corrector, dict):
            self.corrector = corrector_config_from_state(self.corrector)
        if self.include_channel_mask_inputs:
            raise NotImplementedError("include_channel_mask_inputs is outside the accelerated hot path")
        for name in self.prescribed_prognostic_names:
            if name not in self.out_names:
                raise ValueError(f"prescribed_prognostic_name '{name}' must be in out_names: {self.out_names}")
        for name in self.next_step_forcing_names:
            if name not in self.in_names:
                raise ValueError(f"next_step_forcing_name '{name}' not in in_names: {self.in_names}")
            if name in self.out_names:
                raise ValueError(f"next_step_forcing_name is an output variable: '{name}'")
        if self.secondary_decoder is not None:
            for name in self.secondary_decoder.secondary_diagnostic_names:
                if name in self.in_names:
                    raise ValueError(f"secondary_diagnostic_name is an input variable: '{name}'")
                if name in self.out_names:
                    raise ValueError(f"secondary_diagnostic_name is an output variable: '{name}'")

    @property
    def n_ic_timesteps(self) -> int:
        return 1

    @property
    def _normalize_names(self):
        return list(set(self.in_names).union(self.output_names))

    @property
    def input_names(self) -> List[str]:
        if self.ocean is None:
            return self.in_names
        return list(set(self.in_names).union(self.ocean.forcing_names))

    @property
    def output_names(self) -> List[str]:
        """the network's outputs, then the secondary decoder's diagnostics (single_module.py:179-188)"""
        extra = self.secondary_decoder.secondary_diagnostic_names if self.secondary_decoder is not None else []
        return list(self.out_names) + [n for n in extra if n not in self.out_names]

    @property
    def prognostic_names(self) -> List[str]:
        return [n for n in self.out_names if n in self.in_names]

    @property
    def next_step_input_names(self) -> List[str]:
        result = set(self.input_names).difference(self.output_names)
        if self.ocean is not None:
            result = result.union(self.ocean.forcing_names)
        return list(result.union(self.prescribed_prognostic_names))

    def get_next_step_forcing_names(self) -> List[str]:
        return self.next_step_forcing_names

    def get_step(self, dataset_info, init_weights: Callable[[List[nn.Module]], None] = lambda _m: None):
        normalizer = self.normalization.build(self._normalize_names)
        return SingleModuleStep(config=self, dataset_info=dataset_info, normalizer=normalizer,
                                init_weights=init_weights)


def step_with_adjustments(input: TensorMapping, next_step_input_data: TensorMapping,
                          network_calls: Callable[[TensorDict], TensorDict], normalizer: StandardNormalizer,
                          residual_prediction: bool, prognostic_names: List[str],
                          prescribed_prognostic_names: Optional[List[str]] = None,
                          stepper_state=None, corrector=None, ocean=None, global_mean_removal=None,
                          data_mask=None, step_diagnostics: bool = False) -> StepOutput:
    """single_module.py:595-733: (global-mean removal), normalise, network, (residual), denormalise, (global means restored),
    corrector, ocean, prescribed prognostics - in the reference's order (single_module.py:650-716).  The corrector, the ocean and
    the prescribed prognostics see the unshifted input and the physical output.  ``step_diagnostics`` (off by default; the
    reference always does this): ``StepOutput.corrector_diagnostics`` gets ``corrected - output`` of every name the atmosphere
    corrector wrote (single_module.py:669-733), without the prescribed prognostic names; the ocean's surface temperature among
    them raises ``ValueError``."""
    if prescribed_prognostic_names is None:
        prescribed_prognostic_names = []
    gmr_state = None
    if global_mean_removal is not None:
        network_input, gmr_state = global_mean_removal.forward_transform(input, data_mask)
        input_norm = normalizer.normalize(network_input)
        # the synthetic channels are produced in normalised space: merged after the normaliser (single_module.py:656-659)
        input_norm = {**input_norm, **global_mean_removal.extras_normalized(gmr_state)}
    else:
        input_norm = normalizer.normalize(input)
    output_norm = network_calls(input_norm)
    if residual_prediction:
        output_norm = {**output_norm, **{k: input_norm[k] + output_norm[k] for k in prognostic_names}}
    output = normalizer.denormalize(output_norm)
    if global_mean_removal is not None:
        output = global_mean_removal.inverse_transform(output, gmr_state)
    delta: TensorDict = {}
    if corrector is not None:
        cstate = stepper_state.corrector_state if stepper_state is not None else None
        uncorrected = output
        output, cstate = corrector(input, output, next_step_input_data, cstate)
        if step_diagnostics:
            if not hasattr(corrector, "last_modified_names"):
                raise NotImplementedError(f"step_diagnostics: the deltas of {type(corrector).__name__} are not built (only the "
                                          "atmosphere corrector reports them)")
            delta = {n: (output[n] - uncorrected[n]).detach() for n in corrector.last_modified_names}
        if cstate is not None:      # keep the other fields of an incoming state (single_module.py:683-693)
            stepper_state = (StepperState(corrector_state=cstate) if stepper_state is None
                             else dataclasses.replace(stepper_state, corrector_state=cstate))
    if ocean is not None:
        # the ocean writes after the corrector: its name among the deltas would make them inexact (single_module.py:692-706)
        overlap = {ocean.surface_temperature_name} & set(delta)
        if overlap:
            raise ValueError(f"post-corrector adjustment names overlap the corrector's modified names: {sorted(overlap)}")
        output = ocean(input, output, next_step_input_data)
    for name in prescribed_prognostic_names:
        if name in next_step_input_data:
            output = {**output, name: next_step_input_data[name]}
        else:
            raise ValueError(f"prescribed_prognostic_name '{name}' not in next_step_input_data")
    # a prescribed overwrite replaces the output: the corrector's delta no longer describes it (single_module.py:717-728)
    delta = {n: v for n, v in delta.items() if n not in prescribed_prognostic_names}
    return StepOutput(output=output, stepper_state=stepper_state, corrector_diagnostics=delta)


class SingleModuleStep:
    """single_module.py:261-511."""

    TIME_DIM = 1
    CHANNEL_DIM = -3

    def __init__(self, config: SingleModuleStepConfig, dataset_info, normalizer: StandardNormalizer,
                 init_weights: Callable[[List[nn.Module]], None] = lambda _m: None, device=None):
        # global-mean removal (single_module.py:287-298): its synthetic channels are packed after the in_names
        self._global_mean_removal = (config.global_mean_removal.build(normalizer, list(config.in_names))
                                     if config.global_mean_removal is not None else None)
        extra_names = self._global_mean_removal.extra_channel_names if self._global_mean_removal is not None else []
        n_in_channels = len(config.in_names) + len(extra_names)
        n_out_channels = len(config.out_names)
        self.in_packer = Packer(list(config.in_names) + extra_names)
        self.out_packer = Packer(list(config.out_names))
        self._normalizer = normalizer
        module = config.builder.build(n_in_channels=n_in_channels, n_out_channels=n_out_channels,
                                      dataset_info=dataset_info)
        dev = device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu")
        self.module = module.to(dev)
        self.secondary_decoder = (config.secondary_decoder.build(n_in_channels=n_out_channels, dataset_info=dataset_info).to(dev)
                                  if config.secondary_decoder is not None else None)
        init_weights(self.modules)
        self._img_shape = dataset_info.img_shape
        self._config = config
        self._corrector = config.corrector.get_corrector(dataset_info,
                                                         ignore_unsupported=getattr(config, "_ignore_unsupported", False))
        self._ocean = (config.ocean.build(list(config.in_names), list(config.out_names), dataset_info.timestep)
                       if config.ocean is not None else None)
        self._timestep = dataset_info.timestep
        self._vertical_coordinate = getattr(dataset_info, "vertical_coordinate", None)   # derived variables only
        self.in_names = config.in_names
        self.out_names = config.out_names

    @property
    def config(self) -> SingleModuleStepConfig:
        return self._config

    @property
    def normalizer(self) -> StandardNormalizer:
        return self._normalizer

    @property
    def global_mean_removal(self):
        """The step's ``GlobalMeanRemoval`` transform, None without the option."""
        return self._global_mean_removal

    @property
    def input_names(self) -> List[str]:
        return self._config.input_names

    @property
    def output_names(self) -> List[str]:
        return self._config.output_names

    @property
    def prognostic_names(self) -> List[str]:
        return self._config.prognostic_names

    @property
    def next_step_forcing_names(self) -> List[str]:
        return self._config.get_next_step_forcing_names()

    @property
    def next_step_input_names(self) -> List[str]:
        return self._config.next_step_input_names

    @property
    def modules(self) -> nn.ModuleList:
        mods = [self.module.torch_module]
        if self.secondary_decoder is not None:
            mods.extend(self.secondary_decoder.torch_modules)
        return nn.ModuleList(mods)

    def step(self, args: StepArgs, wrapper: Callable[[nn.Module], nn.Module] = lambda x: x,
             step_diagnostics: bool = False) -> StepOutput:
        def network_call(input_norm: TensorDict) -> TensorDict:
            if args.data_mask is not None:
                raise NotImplementedError("data masks are outside the accelerated hot path")
            input_tensor = self.in_packer.pack(input_norm, axis=self.CHANNEL_DIM)
            output_tensor = self.module.wrap_module(wrapper)(input_tensor, labels=args.labels)
            output = self.out_packer.unpack(output_tensor, axis=self.CHANNEL_DIM)
            if self.secondary_decoder is not None:      # column-local diagnostics from the same normalised tensor (single_module.py:430-434)
                output.update(self.secondary_decoder(output_tensor))
            return output

        return step_with_adjustments(
            input=args.input, next_step_input_data=args.next_step_input_data, network_calls=network_call,
            normalizer=self.normalizer, residual_prediction=self._config.residual_prediction,
            prognostic_names=self.prognostic_names,
            prescribed_prognostic_names=self._config.prescribed_prognostic_names,
            stepper_state=args.stepper_state, corrector=self._corrector, ocean=self._ocean,
            global_mean_removal=self._global_mean_removal, data_mask=args.data_mask, step_diagnostics=step_diagnostics,
        )

    def get_state(self):
        return {"module": self.module.get_state(),
                "secondary_decoder": self.secondary_decoder.get_module_state() if self.secondary_decoder is not None else None}

    def load_state(self, state: Dict[str, Any]) -> None:
        module = dict(state["module"])
        if "module.device_buffer" in module:
            del module["module.device_buffer"]
        # checkpoints written through DummyWrapper/DDP carry a "module." prefix (non_distributed.py:15-28); a family whose own keys
        # begin with "module." (AnkurLocalNet's wrapper) keeps them when the state is already its own (this step's get_state)
        own = set(self.module.torch_module.state_dict())
        if module and all(k.startswith("module.") or k == "label_encoding" for k in module) and \
                not {k for k in module if k != "label_encoding"} <= own:
            module = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in module.items()}
        self.module.load_state(module)
        if self.secondary_decoder is not None and state.get("secondary_decoder") is not None:
            self.secondary_decoder.load_module_state(state["secondary_decoder"])
