"""polardepth.functional.side_stream: the streams for side work (the Trainer's encoder streams, the weight-gradient stream, the
attention stream) stay distinct although torch hands out its 32 pool streams round-robin.  A process that builds many Trainers
was otherwise given the weight-gradient stream as an encoder stream; inside a captured step that stream then waited for its own
event, and ending the capture crashed."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_side_streams_stay_distinct_over_more_than_one_round_of_the_pool():
    from polardepth import functional as PF
    dev = torch.device("cuda", torch.cuda.current_device())
    wgrad, attn, cur = PF.wgrad_stream(dev), PF._attn_side_stream(dev), torch.cuda.current_stream(dev)
    assert wgrad != attn and wgrad != cur and attn != cur
    assert PF.wgrad_stream(dev) is wgrad and PF._attn_side_stream(dev) is attn
    capture = torch.cuda.graph.default_capture_stream          # None until this process has captured a graph
    drawn = []
    for _ in range(70):                                        # the pool wraps twice
        st = PF.side_stream(dev, drawn[-1:] + [cur])
        assert st not in (wgrad, attn, capture, cur) and st not in drawn[-1:]
        drawn.append(st)
    held = {s.cuda_stream for s in (wgrad, attn, capture) if s is not None}
    assert len({s.cuda_stream for s in drawn}) == 32 - len(held)       # every pool stream but the long-lived ones


def test_side_stream_says_so_when_every_pool_stream_is_taken():
    from polardepth import functional as PF
    dev = torch.device("cuda", torch.cuda.current_device())
    pool = [torch.cuda.Stream(device=dev) for _ in range(32)]
    assert len({s.cuda_stream for s in pool}) == 32
    with pytest.raises(RuntimeError, match="pool streams"):
        PF.side_stream(dev, pool)


def test_a_trainers_encoder_streams_avoid_the_weight_gradient_stream(tmp_path, monkeypatch):
    from test_step_gpu import _opts
    from manydepth.trainer import Trainer
    from polardepth import functional as PF
    tr = Trainer(_opts(tmp_path, ["--dropout_rate", "0.0"]))
    monkeypatch.setattr(PF, "register_producer_stream", lambda st: None)      # (these streams produce nothing)
    wgrad = PF.wgrad_stream(tr.device)
    for _ in range(40):                                        # as if 20 Trainers had drawn their two streams before
        tr._enc_streams = []
        a, b = tr._encoder_stream(0), tr._encoder_stream(1)
        assert a != b and wgrad not in (a, b) and torch.cuda.current_stream(tr.device) not in (a, b)
