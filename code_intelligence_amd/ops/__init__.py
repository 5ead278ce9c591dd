"""HIP/CDNA4 op layer: dispatch between gfx950 kernels (ROCm) and the
pure-PyTorch CPU reference implementations. See SURVEY.md §2.4 for the
kernel inventory (K1-K9); K10 (decode-and-sample) and K11 (beam search) are
in ARCHITECTURE.md."""
from . import extension
from .lstm import lstm_forward
from .pool import concat_pool, StreamingConcatPool, pool_head
from .dropout import variational_dropout
from .crossentropy import tied_decoder_ce, TiedDecoderCE
from .adam import FusedAdamW
from .decode import decode_cutoff, decode_logits, sample_next
from .beam import topk_logprobs, beam_select

__all__ = [
    "extension", "lstm_forward", "concat_pool", "StreamingConcatPool",
    "pool_head", "variational_dropout",
    "tied_decoder_ce", "TiedDecoderCE", "FusedAdamW",
    "decode_logits", "decode_cutoff", "sample_next", "topk_logprobs", "beam_select",
]
