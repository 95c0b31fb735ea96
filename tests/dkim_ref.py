"""TEST INFRASTRUCTURE: a literal Python restatement of the reference's DKIM canonicalisers (packages/helpers/src/lib/mailauth), the
yardstick of tests/test_dkim_cpu.py and tests/test_dkim_gpu.py.  Not product code; nothing here is imported by zkwg.

  relaxed_body   body/relaxed.ts: fixLineBuffer (:113-155) on every line, pushBodyHash's queue of line ends and empty lines (:84-111),
                 the closing CR LF of a non-empty body (:261-264) and l= (updateBodyHash, :46-73).
                 NOT restated: the scan of update() (:185-235) that decides which lines go through fixLineBuffer at all.  It is a
                 shortcut for lines that are canonical already, and it misses some that are not -- `SP CR CR LF` (:188-196), and a
                 single SP or a CR at the end of a last line without line end (:255-259).  Here every line is fixed.
  simple_body    body/simple.ts: update (:59-97) with the whole body as one chunk, digest (:99-106), l= (:36-57)
  parse_headers  tools.ts:75-105
  signing_lines  tools.ts:107-140 (verify = true)
  relaxed_header header/relaxed.ts:20-78 with formatRelaxedLine (tools.ts:441-454)
  simple_header  header/simple.ts:23-83
"""
import re

CR, LF, SP, TAB = 13, 10, 32, 9


class _Body:
    def __init__(self, max_body_length):
        self.max = max_body_length           # a number, or None ('' in dkim-verifier.ts:141-144)
        self.hashed = 0
        self.full = bytearray()
        self.max_reached = False


class _Relaxed(_Body):
    def __init__(self, max_body_length):
        super().__init__(max_body_length)
        self.queue = []

    def update_body_hash(self, chunk):                   # relaxed.ts:46-73
        if self.max_reached:
            return
        if self.max is not None and self.max >= 0 and self.hashed + len(chunk) > self.max:
            self.max_reached = True
            if self.hashed >= self.max:
                return
            chunk = chunk[:self.max - self.hashed]
        self.hashed += len(chunk)
        self.full += chunk

    def drain(self):                                     # relaxed.ts:75-82
        for e in self.queue:
            self.update_body_hash(e)
        self.queue = []

    def push_body_hash(self, chunk):                     # relaxed.ts:84-111
        if not chunk:
            return
        found = False
        for i in range(len(chunk) - 1, -1, -1):
            if chunk[i] != LF and chunk[i] != CR:
                self.drain()
                if i < len(chunk) - 1:
                    self.queue.append(chunk[i + 1:])
                    chunk = chunk[:i + 1]
                found = True
                break
        if not found:
            self.queue.append(chunk)
            return
        self.update_body_hash(chunk)


def fix_line_buffer(line):                               # relaxed.ts:113-155
    out = []
    non_wsp_found = prev_wsp = False
    for i in range(len(line) - 1, -1, -1):
        if line[i] == LF:
            out.insert(0, line[i])
            if i == 0 or line[i - 1] != CR:
                out.insert(0, CR)
            continue
        if line[i] == CR:
            out.insert(0, line[i])
            continue
        if line[i] == SP or line[i] == TAB:
            if non_wsp_found:
                prev_wsp = True
            continue
        if prev_wsp:
            out.insert(0, SP)
            prev_wsp = False
        non_wsp_found = True
        out.insert(0, line[i])
    if prev_wsp and non_wsp_found:
        out.insert(0, SP)
    return bytes(out)


def relaxed_body(body, l=None):
    h = _Relaxed(l)
    pos = 0
    while pos < len(body):
        end = body.find(b"\n", pos)
        end = len(body) if end < 0 else end + 1
        if not h.max_reached:                            # relaxed.ts:159-161
            h.push_body_hash(fix_line_buffer(body[pos:end]))
        pos = end
    if h.hashed:                                         # relaxed.ts:261-264
        h.update_body_hash(b"\r\n")
    return bytes(h.full)


def simple_body(body, l=None):
    h = _Body(l)
    remainder = []
    last_newline = False

    def update_body_hash(chunk):                         # simple.ts:36-57
        if h.max is not None and h.max >= 0 and h.hashed + len(chunk) > h.max:
            if h.hashed >= h.max:
                return
            chunk = chunk[:h.max - h.hashed]
        h.hashed += len(chunk)
        h.full += chunk

    chunk = body                                         # simple.ts:59-97, one chunk
    if len(chunk):
        match_start = None
        for i in range(len(chunk) - 1, -1, -1):
            if chunk[i] in (LF, CR):
                match_start = i
            else:
                break
        if match_start == 0:
            remainder.append(chunk)
        else:
            if match_start is not None:
                remainder.append(chunk[match_start:])
                chunk = chunk[:match_start]
            update_body_hash(chunk)
            last_newline = chunk[-1] == LF
    if not last_newline or not h.hashed:                 # simple.ts:99-106
        update_body_hash(b"\r\n")
    return bytes(h.full)


def body_offset(raw):                                    # message-parser.ts:50-76
    for i in range(1, len(raw)):
        if raw[i] == LF and (raw[i - 1] == LF or (i >= 2 and raw[i - 1] == CR and raw[i - 2] == LF)):
            return i + 1
    return len(raw)


def parse_headers(buf):                                  # tools.ts:75-105 -> [(key, casedKey, line)]
    rows = [[r] for r in re.split(r"\r?\n", re.sub(r"[\r\n]+$", "", buf.decode("latin-1")))]
    for i in range(len(rows) - 1, -1, -1):
        if i > 0 and re.match(r"^\s", rows[i][0]):
            rows[i - 1] = rows[i - 1] + rows[i]
            del rows[i]
    out = []
    for row in rows:
        s = "\r\n".join(row)
        m = re.match(r"^[^:]+", s)
        cased = m.group(0).strip() if m else None
        out.append((cased.lower() if m else None, cased, s.encode("latin-1")))
    return out


def signing_lines(parsed, field_names):                  # tools.ts:107-140, verify
    names = [k.strip().lower() for k in field_names.split(":")]
    names = [k for k in names if k]
    left = list(parsed)
    out = []
    for name in names:
        for i in range(len(left) - 1, -1, -1):
            if name == left[i][0]:
                out.append(left[i])
                del left[i]
                break
    return out


def format_relaxed_line(line, suffix=""):                # tools.ts:441-454
    s = re.sub(r"\r?\n", "", line.decode("latin-1"))
    s = re.sub(r"^([^:]*):\s*", lambda m: m.group(1).lower().strip() + ":", s, count=1)
    s = re.sub(r"\s+", " ", s).strip()
    return (s + suffix).encode("latin-1")


def _empty_b(line):                                      # header/relaxed.ts:75, header/simple.ts:78
    return re.sub(r"([;:\s]+b=)[^;]+", r"\1", line.decode("latin-1"), count=1).encode("latin-1")


def relaxed_header(lines, signature_line):               # header/relaxed.ts:20-78
    return b"".join(format_relaxed_line(l[2], "\r\n") for l in lines) + _empty_b(format_relaxed_line(signature_line))


def simple_header(lines, signature_line):                # header/simple.ts:23-83
    return b"".join(l[2] + b"\r\n" for l in lines) + _empty_b(signature_line)
