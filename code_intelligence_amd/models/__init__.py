from .awd_lstm import (AWDLSTM, AWDLSTMEncoder, EmbeddingDropout,
                       LinearDecoder, RNNDropout, WeightDroppedLSTM,
                       WeightDroppedQRNN, awd_lstm_lm_config)
from .classifier import (MultiBatchEncoder, PoolingLinearClassifier,
                         TextClassifier, awd_lstm_clas_config,
                         get_text_classifier)

__all__ = [
    "AWDLSTM", "AWDLSTMEncoder", "EmbeddingDropout", "LinearDecoder",
    "RNNDropout", "WeightDroppedLSTM", "WeightDroppedQRNN",
    "awd_lstm_lm_config",
    "MultiBatchEncoder", "PoolingLinearClassifier", "TextClassifier",
    "awd_lstm_clas_config", "get_text_classifier",
]
