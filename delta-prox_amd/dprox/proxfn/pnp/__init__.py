from .denoisers import Denoiser, Denoiser2D, DRUNetDenoiser, FFDNet, FFDNetColorDenoiser, FFDNetDenoiser, GRUnet, GRUNetDenoiser, GRUNetTVDenoiser, IRCNN, IRCNNDenoiser, QRNN3DDenoiser, TVDenoiser, UNet, UNetDenoiser, UNetRes
from .prior import deep_prior, get_denoiser
