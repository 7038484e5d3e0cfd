"""``rank_print`` hands a whole line to the stream in one write: the ranks of a job share one
pipe, and the launcher tests parse rank 0's summary line off it."""
import io
import sys

from distributed_training_pytorch_amd.utils.logging import rank_print


class _Raw(io.RawIOBase):
    def __init__(self):
        self.calls = []

    def writable(self):
        return True

    def write(self, b):
        self.calls.append(bytes(b))
        return len(b)


def test_rank_print_is_one_write_on_an_unbuffered_stream(monkeypatch):
    """What ``python -u`` / PYTHONUNBUFFERED gives: a write-through text layer over a raw file.
    There ``print(a, b)`` is four writes (a, the separator, b, the newline), between which
    another rank's text can land."""
    raw = _Raw()
    monkeypatch.setattr(sys, "stdout", io.TextIOWrapper(raw, write_through=True))
    rank_print(1, "summary:", {"iters": 20, "final_loss": [1.5, 2.5]})
    assert raw.calls == [b"[Process 1] summary: {'iters': 20, 'final_loss': [1.5, 2.5]}\n"]
    raw.calls.clear()
    print("[Process 1]", "Finished", flush=True)
    assert len(raw.calls) == 4  # the premise: this is what the line was before
