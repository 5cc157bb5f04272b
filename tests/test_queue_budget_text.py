"""What a value of GPU_MAX_HW_QUEUES resolves to as the library's queue budget (nxhip_queue_budget_from_text): the parser alone, on
text handed to it — no device, and the environment of the process is never touched."""
import pytest

from nexus_amd import capi


@pytest.mark.parametrize("text,want", [
    (None, 4), ("", 4),                                   # not set, or empty: the runtime's own default
    ("1", 1), ("4", 4), ("7", 7), ("24", 24), ("32", 32),  # a whole number in [1, 32] is itself
    ("0", 4), ("33", 4), ("64", 4), ("-3", 4), ("99999999999999999999", 4),  # out of range
    ("many", 4), ("4x", 4), ("8 ", 4), ("3.5", 4), ("0x10", 4),              # not a whole number from end to end
])
def test_text_resolves_to_the_budget(text, want):
    assert capi.queue_budget_from_text(text) == want
