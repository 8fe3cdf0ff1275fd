"""BankAccount state-topic partitions for the string-column tests: what ``tests/state_topic_gen.py`` does for the Counter
model, with the docs' model — UUID keys, Double text and the two string fields the decoder has to keep.

Built on ``state_topic_gen.batch`` / ``compacted_batch`` (offset gaps, LZ4 or none, transactions with their markers, the
producer's leading flush record).  Owners carry what a JSON string can: quotes, backslashes, ``/``, tab and newline, 2-, 3-
and 4-byte UTF-8; a value is written with ``ensure_ascii=False`` (Jackson's form: non-ASCII raw) or, where the owner has no
character beyond the BMP, sometimes with ``ensure_ascii=True`` (every non-ASCII character a ``\\uXXXX``).  Security codes
are empty for some accounts.  Ids are tombstoned and re-created under another owner.  ``make_topic`` returns the units per
partition and its OWN last-wins table ``{id: (owner, code, balance) | None}``."""
import json
import uuid

import numpy as np

from kafka_wire import COMMIT, control_batch
from state_topic_gen import compacted_batch, concat, split  # noqa: F401  (concat / split: re-exported for the tests)
from surge_amd.encode import play_json_double

OWNERS = ("Jane Doe", 'Ann "Q" O\'Neil', "back\\slash / slash", "tab\there", "line\nbreak", "Zoë Ñandú", "€uro 漢字", "smile 😀 end", "", "x",
          '"', "\\", "é", "ends with quote\"", "\ttab first")


def state_text(account_id: str, owner: str, code: str, balance: float, ascii_only: bool = False) -> bytes:
    q = lambda v: json.dumps(v, ensure_ascii=ascii_only)  # noqa: E731
    return (f'{{"accountNumber":{q(account_id)},"accountOwner":{q(owner)},"securityCode":{q(code)},'
            f'"balance":{play_json_double(balance)}}}').encode("utf-8")


def make_topic(seed=5, n_ids=150, n_records=800, n_partitions=2, compression="lz4"):
    rng = np.random.default_rng(seed)
    ids = [str(uuid.UUID(int=int(rng.integers(1, 2 ** 62)) * 7919 + i)) for i in range(n_ids)]
    table = {}
    life = [0] * n_ids  # how often the id was (re-)created
    units = [[] for _ in range(n_partitions)]
    next_off = [int(rng.integers(0, 1000)) for _ in range(n_partitions)]
    made, first = 0, True
    while made < n_records:
        p = int(rng.integers(0, n_partitions))
        recs, delta = [], int(rng.integers(0, 3))
        for _ in range(int(rng.integers(1, 30))):
            i = int(rng.integers(0, n_ids // n_partitions)) * n_partitions + p
            if i >= n_ids:
                i = p
            key = ids[i]
            if table.get(key) is not None and rng.random() < 0.25:
                table[key] = None
                value = None
            else:
                if table.get(key) is None:  # created, or re-created under another owner
                    life[i] += 1
                    owner = OWNERS[(i + 3 * life[i]) % len(OWNERS)] + (f" #{life[i]}" if life[i] > 1 and i % 2 else "")
                    code = "" if i % 5 == 0 else f"{(i * 7919) % 10000:04d}"
                else:
                    owner, code, _ = table[key]
                balance = float(int(rng.integers(-10 ** 6, 10 ** 6))) / 100.0 or 1.0
                table[key] = (owner, code, balance)
                bmp = all(ord(ch) < 0x10000 for ch in owner)
                value = state_text(key, owner, code, balance, ascii_only=bmp and rng.random() < 0.4)
            recs.append((delta, key.encode("ascii"), value))
            delta += 1 + int(rng.integers(0, 3)) * (rng.random() < 0.3)
        data = b""
        if first:  # the producer's flush record leads the topic, in a transaction of its own
            first = False
            b, _, next_off[p] = compacted_batch(next_off[p], [(0, b"", b"")], compression, transactional=True, producer_id=7)
            data += b + control_batch(next_off[p], 7, COMMIT)
            next_off[p] += 1
        txn = rng.random() < 0.4
        b, delivered, next_off[p] = compacted_batch(next_off[p], recs, compression, tail_gap=int(rng.integers(0, 3)),
                                                    **({"transactional": True, "producer_id": 7} if txn else {}))
        data += b
        if txn:
            data += control_batch(next_off[p], 7, COMMIT)
            next_off[p] += 1
        made += len(delivered)
        units[p].append((data, delivered))
    return units, table
