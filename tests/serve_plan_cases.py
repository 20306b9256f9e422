"""What a serving slot must plan to launch (ext.ServeSlot.plan), restated
from the rules in docs/DESIGN.md ("Serving plan") independently of the C++
that decides it. Shared by tests/test_gpu_serve_plan.py and the two
test_switch_parity tests."""


def wstat_pays(B: int, cus: int) -> bool:
    """xg_gemm4w_pays(90 * B): whole 256-row tiles, and at least eight of
    them for each of the 8 * (CUs per XCD // 6) walkers of one n-tile. On
    256 CUs: B % 128 == 0 and B >= 1024."""
    M = 90 * B
    walkers = max(1, 8 * (cus // 8 // 6))
    return M % 256 == 0 and M // 256 >= 8 * walkers


def expected_plan(B: int, cus: int, env=None) -> dict:
    """The plan of a slot of B rows built from _bf16_weights (padded widths
    512/256/256) with the ROKO_* switches in `env` and no others set."""
    env = env or {}
    front = env.get("ROKO_FRONT")
    front = "v4" if front in (None, "v4") else "v2" if front == "v2" else "v3"
    fold = env.get("ROKO_XGFOLD") == "1"
    raw = fold or (env.get("ROKO_XG2") != "0" and B % 128 == 0)
    plan = {"front": front, "xg": ["lt"] * 3, "seq_ld": 500, "raw": raw,
            "graph": False}
    if not raw:
        return plan
    gslot = env.get("ROKO_GSLOT")
    plan["graph"] = gslot == "1" if gslot is not None else B >= 256
    if fold:
        plan["xg"] = ["fold"] * 3
    elif env.get("ROKO_XG3") == "0" or front == "v2":
        plan["xg"] = ["xg2"] * 3
    else:
        plan["seq_ld"] = 512
        xg4 = env.get("ROKO_XG4")
        if xg4 == "0":
            plan["xg"] = ["xg3"] * 3
        elif xg4 == "stream":
            plan["xg"] = ["stream"] * 3
        else:
            wide = (90 * B) % 256 == 0 if xg4 == "wstat" else wstat_pays(B, cus)
            plan["xg"] = ["xg3"] + ["wstat" if wide else "xg3"] * 2
    return plan
