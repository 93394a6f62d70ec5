"""MI355X-native (gfx950) Ctrl-Adapter denoising hot path: ControlNet + Ctrl-Adapter (+ router) forward behind the
reference's own module interface.  All arithmetic runs in libctrlhip.so (hand-written HIP); see DESIGN.md."""
from . import _lib  # noqa: F401
from .controlnet import ControlNetModel, ControlNetOutput, MultiControlNetModel, pool_latents  # noqa: F401
from .ctrl_adapter import ControlNetAdapter  # noqa: F401
from .ctrl_router import ControlNetRouter  # noqa: F401
from .fused import controlled_step  # noqa: F401
from .image_prep import prepare_images  # noqa: F401
from .canny import canny, extract_canny  # noqa: F401  (the name `canny` is the function; the module stays importable as ctrl_adapter_amd.canny)
from .hed import HEDdetector, extract_scribble, extract_softedge  # noqa: F401
from .pidinet import PidiNetDetector, pidinet_state_dict_spec  # noqa: F401
from .lineart import LineartDetector, extract_lineart, lineart_state_dict_spec  # noqa: F401
from .text_encoder import CLIPTextModel, CLIPTextOutput, encode_controlnet_prompt  # noqa: F401
from .text_encoder import CLIPTextModelWithProjection, CLIPTextModelOutput, encode_sdxl_prompt  # noqa: F401
from .vision_encoder import CLIPVisionModelWithProjection, CLIPVisionModelOutput, encode_i2vgen_image, encode_svd_image  # noqa: F401
from .vae_encoder import AutoencoderKLEncoder, encode_svd_image_latents, prepare_i2vgen_image_latents  # noqa: F401
from .vae_decoder import AutoencoderKL, AutoencoderKLDecoder, DecoderOutput, decode_i2vgen_latents, decode_sdxl_latents  # noqa: F401
from .vae_temporal_decoder import AutoencoderKLTemporalDecoder, decode_svd_latents  # noqa: F401
from .unet_spatio_temporal import UNetSpatioTemporalConditionModel, UNetSpatioTemporalConditionOutput  # noqa: F401
from .unet_2d_condition import UNet2DConditionModel, UNet2DConditionOutput  # noqa: F401
from .unet_i2vgen_xl import I2VGenXLUNet, UNet3DConditionOutput  # noqa: F401
from .schedulers import DDIMScheduler, EulerDiscreteScheduler, SchedulerOutput  # noqa: F401
from .denoise import DenoiseLoop, denoise_svd  # noqa: F401
