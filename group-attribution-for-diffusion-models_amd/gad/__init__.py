"""gad - MI355X-native (gfx950) hot path of the Shapley data-attribution engine.

The names exported here are the ones the reference takes from `diffusers`
(main.py:22-24, src/diffusion_utils.py:15-23): entry points import this module in place of
diffusers for the objects on the hot path."""
from . import _capi, ops  # noqa: F401
from .ops import operand_precision, set_operand_precision  # noqa: F401
from .nn import LoRALinearLayer, UNet2DModel  # noqa: F401
from .pipelines import DDIMPipeline, DDPMPipeline, LDMPipeline, StableDiffusionLatentPipeline, sd_simple_loss  # noqa: F401
from .schedulers import DDIMScheduler, DDPMScheduler, PNDMScheduler, sd_scheduler  # noqa: F401
from .training import EMAModel, FusedTrainer, adam8_blocks, flatten_params, lr_lambda  # noqa: F401
from . import coalition  # noqa: F401,E402
from .coalition import DeviceLoader, antithetic_timesteps, seed_everything  # noqa: F401,E402

__version__ = "0.1.0"
from .scoring import diversity_against_dataset, fid_against_dataset, global_scores_against_dataset  # noqa: F401,E402
from .sd import UNet2DConditionModel  # noqa: F401,E402
from .local import LocalBehaviors, local_model_behaviors  # noqa: F401,E402
from .influence import InfluenceUnlearner  # noqa: F401,E402
from .lora import LoraConfig, get_peft_model, lora_parameters, merge_and_unload  # noqa: F401,E402
from .similarity import cosine_rows, group_aggregate, write_baselines  # noqa: F401,E402
from .vae import AutoencoderKL, VQModel  # noqa: F401,E402
from .text import CLIPTextModel, CLIPTokenizer, TextTower  # noqa: F401,E402
from .latents import MomentSource  # noqa: F401,E402
