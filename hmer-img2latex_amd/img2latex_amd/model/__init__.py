"""Same public names as the reference's img2latex.model (model/__init__.py:1-3), plus this package's ensemble."""
from .cnn_encoder import CNNEncoder
from .lstm_decoder import Attention, LSTMDecoder
from .resnet_encoder import ResNetEncoder
from .seq2seq_model import BeamHypothesis, SampleHypothesis, Seq2SeqModel
from .ensemble import EnsembleDecoder, EnsembleModel

__all__ = ["CNNEncoder", "ResNetEncoder", "LSTMDecoder", "Attention", "Seq2SeqModel", "BeamHypothesis", "SampleHypothesis",
           "EnsembleDecoder", "EnsembleModel"]
