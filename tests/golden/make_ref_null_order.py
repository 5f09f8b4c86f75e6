"""Transcribes ORDER BY cases over nullable keys from the reference's SQL-level suite (test/sqlite-small/unnesting.test) into an
operator-level fixture: the table the query reads (parsed from its INSERT statement), and the result rows in the order the reference
expects them (parsed from the lines under `----`).  Taken are the live (not commented-out) blocks
  * `SELECT i, … FROM integers i1 ORDER BY i;`  over integers(i) = 1, 2, 3, NULL: the sort key is result column 0, the NULL row comes last;
    many of them have a second column that is NULL for every row, or for some,
  * `SELECT * FROM strings … ORDER BY v;`       over strings(v) = 'hello', 'world', NULL,
  * the one `ORDER BY … LIMIT` statement that orders a nullable key (over the empty table item: `statement ok`, no rows).
Every value is an int, a string, true / false (the `t` / `f` of a boolean column) or null.  A `key_type` of "int32" / "utf8" says how the
sort key (column 0) is to be built.  Writes ref_null_order.json.  Needs /root/reference."""
import json
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = "/root/reference/test/sqlite-small/unnesting.test"
INTEGERS = re.compile(r"^SELECT i, .* FROM integers i1 ORDER BY i;$")
STRINGS = re.compile(r"^SELECT \* FROM strings .*ORDER BY v;$")
LIMIT = re.compile(r"^SELECT \* FROM item i1 .* ORDER BY 1 LIMIT (\d+);$")


def value(text):
    if text == "NULL":
        return None
    if text in ("t", "f"):
        return text == "t"
    return int(text) if re.fullmatch(r"-?\d+", text) else text


def inserted(lines, table):
    """the rows of `INSERT INTO table VALUES (a), (b), …` (one column)"""
    for ln in lines:
        m = re.match(r"INSERT INTO %s VALUES (.*);" % table, ln)
        if m:
            return [value(v.strip().strip("'")) for v in re.findall(r"\(([^()]*)\)", m.group(1))]
    raise SystemExit("no INSERT INTO " + table)


def main():
    lines = open(SRC).read().split("\n")
    tables = {"integers": inserted(lines, "integers"), "strings": inserted(lines, "strings"), "item": []}
    cases = []
    for i, ln in enumerate(lines):
        if ln.startswith("query ") and lines[i + 2] == "----":
            sql = lines[i + 1]
            table = "integers" if INTEGERS.match(sql) else "strings" if STRINGS.match(sql) else None
            if table is None:
                continue
            rows, j = [], i + 3
            while j < len(lines) and lines[j].strip():
                rows.append([value(c) for c in lines[j].split("\t")])
                j += 1
            cases.append({"source": "test/sqlite-small/unnesting.test:%d" % (i + 2), "sql": sql, "table": table, "input": tables[table],
                          "key_type": "int32" if table == "integers" else "utf8", "limit": None, "expected": rows})
        elif ln == "statement ok" and LIMIT.match(lines[i + 1]):
            cases.append({"source": "test/sqlite-small/unnesting.test:%d" % (i + 2), "sql": lines[i + 1], "table": "item", "input": [], "key_type": "int32",
                          "limit": int(LIMIT.match(lines[i + 1]).group(1)), "expected": []})
    with open(os.path.join(HERE, "ref_null_order.json"), "w") as f:
        json.dump(cases, f, indent=1)
    all_null = sum(1 for c in cases if c["expected"] and len(c["expected"][0]) > 1 and all(r[1] is None for r in c["expected"]))
    print(len(cases), "cases,", all_null, "with an all-NULL second column,", sum(1 for c in cases if c["limit"] is not None), "with LIMIT")


if __name__ == "__main__":
    main()
