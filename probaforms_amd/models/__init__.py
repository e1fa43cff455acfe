"""`from probaforms_amd.models import RealNVP` mirrors `from probaforms.models import RealNVP`
(/root/reference/probaforms/models/__init__.py:1, README.md:48).  The RealNVP path (SURVEY.md
section 8), CVAE, ConditionalWGAN (libpf_wgan.so) and ConditionalNormal
(libpf_cnormal.so) are rebuilt: every model `probaforms.models` exports."""
from .interfaces import GenModel
from .nflow import InvertibleLayer, NormalizingFlow, StandardNormalPrior
from .realnvp import RealNVP, RealNVPLayer, gen_network
from .cvae import CVAE, Decoder, Encoder
from .wgan import ConditionalWGAN, Discriminator, Generator
from .cnormal import ConditionalNormal, Net

__all__ = ['RealNVP', 'CVAE', 'Encoder', 'Decoder', 'ConditionalWGAN', 'Generator', 'Discriminator', 'ConditionalNormal', 'Net', 'RealNVPLayer', 'NormalizingFlow', 'InvertibleLayer', 'GenModel', 'gen_network',
           'StandardNormalPrior']
