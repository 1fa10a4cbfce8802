// nmn_engine_filter.cpp — FilterCondition on the host: the evaluator the reference walks per key (evaluate_filter), its
// translation into a predicate program for the metadata columns on the GPU (compile_filter), the strategy choice of the filtered
// searches and the nmn_filter_* constructors.
#include "nmn_engine_internal.h"

namespace nmn {
namespace engine {

// compare_tensor_value_to_filter (lib.rs:3648-3670): ordering if the types are compatible.
// returns false when incomparable; *ord = -1/0/+1 otherwise.
static bool compare_values(const Value& stored, const Value& flt, int* ord) {
    auto cmp3 = [](auto a, auto b) { return a < b ? -1 : (a > b ? 1 : 0); };
    if (stored.kind == NMN_VAL_INT && flt.kind == NMN_VAL_INT) { *ord = cmp3(stored.i, flt.i); return true; }
    if (stored.kind == NMN_VAL_FLOAT && flt.kind == NMN_VAL_FLOAT) {
        if (std::isnan(stored.f) || std::isnan(flt.f)) return false;  // partial_cmp -> None
        *ord = cmp3(stored.f, flt.f); return true;
    }
    if (stored.kind == NMN_VAL_FLOAT && flt.kind == NMN_VAL_INT) {
        if (std::isnan(stored.f)) return false;
        *ord = cmp3(stored.f, (double)flt.i); return true;
    }
    if (stored.kind == NMN_VAL_INT && flt.kind == NMN_VAL_FLOAT) {
        if (std::isnan(flt.f)) return false;
        *ord = cmp3((double)stored.i, flt.f); return true;
    }
    if (stored.kind == NMN_VAL_STRING && flt.kind == NMN_VAL_STRING) { *ord = cmp3(stored.s.compare(flt.s), 0); return true; }
    if (stored.kind == NMN_VAL_BOOL && flt.kind == NMN_VAL_BOOL) { *ord = cmp3((int)stored.b, (int)flt.b); return true; }
    if (stored.kind == NMN_VAL_NULL && flt.kind == NMN_VAL_NULL) { *ord = 0; return true; }
    return false;
}

// evaluate_filter (lib.rs:3592-3630)
bool evaluate_filter(const Meta& meta, const nmn_filter& f) {
    switch (f.kind) {
        case nmn_filter::True: return true;
        case nmn_filter::And: return evaluate_filter(meta, *f.a) && evaluate_filter(meta, *f.b);
        case nmn_filter::Or: return evaluate_filter(meta, *f.a) || evaluate_filter(meta, *f.b);
        case nmn_filter::Exists: return meta.count(f.field) != 0;
        case nmn_filter::Cmp: {
            auto it = meta.find(f.field);
            if (it == meta.end()) return false;
            int ord = 0;
            if (!compare_values(it->second, f.value, &ord)) return false;
            switch (f.op) {
                case NMN_OP_EQ: return ord == 0;
                case NMN_OP_NE: return ord != 0;
                case NMN_OP_LT: return ord < 0;
                case NMN_OP_LE: return ord <= 0;
                case NMN_OP_GT: return ord > 0;
                default: return ord >= 0;
            }
        }
        case nmn_filter::Contains: {
            auto it = meta.find(f.field);
            return it != meta.end() && it->second.kind == NMN_VAL_STRING && it->second.s.find(f.text) != std::string::npos;
        }
        case nmn_filter::StartsWith: {
            auto it = meta.find(f.field);
            return it != meta.end() && it->second.kind == NMN_VAL_STRING && it->second.s.compare(0, f.text.size(), f.text) == 0;
        }
        case nmn_filter::In: {
            auto it = meta.find(f.field);
            if (it == meta.end()) return false;
            for (const auto& v : f.values) {
                int ord = 0;
                if (compare_values(it->second, v, &ord) && ord == 0) return true;
            }
            return false;
        }
    }
    return false;
}

// ---- FilterCondition -> predicate program (include/neumann_gpu.h, NMN_PRED_*) ------------------------
static nmn_pred_op make_op(uint32_t op, uint32_t column = 0, uint32_t cmp = 0, uint32_t vkind = 0, uint64_t a = 0, uint64_t b = 0) {
    nmn_pred_op o;
    o.op = op;
    o.cmp = cmp;
    o.vkind = vkind;
    o.column = column;
    o.a = a;
    o.b = b;
    return o;
}

// the (kind, payload) a FilterValue compares as; strings never get here
static bool filter_value_cell(const Value& v, uint32_t* kind, uint64_t* payload) {
    *payload = 0;
    switch (v.kind) {
        case NMN_VAL_NULL: *kind = NMN_CELL_NULL; return true;
        case NMN_VAL_BOOL: *kind = NMN_CELL_BOOL; *payload = v.b ? 1 : 0; return true;
        case NMN_VAL_INT: *kind = NMN_CELL_INT; memcpy(payload, &v.i, 8); return true;
        case NMN_VAL_FLOAT: *kind = NMN_CELL_FLOAT; memcpy(payload, &v.f, 8); return true;
        default: return false;
    }
}

// bitset over the dictionary ids of one string column: bit i = test(strings[i])
template <typename Test>
static nmn_pred_op string_set(const FieldColumn& fc, Program& p, Test test) {
    const uint64_t n = fc.strings.size(), off = p.consts.size();
    p.consts.resize(off + (n + 63) / 64, 0ull);
    for (uint64_t i = 0; i < n; i++)
        if (test(fc.strings[i])) p.consts[off + (i >> 6)] |= 1ull << (i & 63);
    return make_op(NMN_PRED_STRSET, fc.id, 0, 0, off, n);
}

// Postfix code of a condition.  And/Or are pure here, so the deeper operand is emitted first
// (Sethi-Ullman order): the stack need grows with log2 of the leaf count, not with the nesting depth.
Code compile_filter(const nmn_filter& f, const Mirror& m, Program& p) {
    Code c;
    auto field = [&](const std::string& name) -> const FieldColumn* {
        auto it = m.fields.find(name);
        return it == m.fields.end() ? nullptr : &it->second;
    };
    switch (f.kind) {
        case nmn_filter::True: c.ops.push_back(make_op(NMN_PRED_TRUE)); return c;
        case nmn_filter::And:
        case nmn_filter::Or: {
            Code a = compile_filter(*f.a, m, p), b = compile_filter(*f.b, m, p);
            if (a.need < b.need) std::swap(a, b);
            c.ops = std::move(a.ops);
            c.ops.insert(c.ops.end(), b.ops.begin(), b.ops.end());
            c.ops.push_back(make_op(f.kind == nmn_filter::And ? NMN_PRED_AND : NMN_PRED_OR));
            c.need = std::max(a.need, b.need + 1);
            return c;
        }
        default: break;
    }
    const FieldColumn* fc = field(f.field);
    if (!fc) {  // no mirrored row has the field: `tensor.get(..)` is None for every row
        c.ops.push_back(make_op(NMN_PRED_FALSE));
        return c;
    }
    switch (f.kind) {
        case nmn_filter::Exists: c.ops.push_back(make_op(NMN_PRED_EXISTS, fc->id)); break;
        case nmn_filter::Contains:
            c.ops.push_back(string_set(*fc, p, [&](const std::string& s) { return s.find(f.text) != std::string::npos; }));
            break;
        case nmn_filter::StartsWith:
            c.ops.push_back(string_set(*fc, p, [&](const std::string& s) { return s.compare(0, f.text.size(), f.text) == 0; }));
            break;
        case nmn_filter::Cmp:
            if (f.value.kind == NMN_VAL_STRING) {
                const int op = f.op;
                c.ops.push_back(string_set(*fc, p, [&](const std::string& s) {
                    const int ord = s.compare(f.value.s);
                    switch (op) {
                        case NMN_OP_EQ: return ord == 0;
                        case NMN_OP_NE: return ord != 0;
                        case NMN_OP_LT: return ord < 0;
                        case NMN_OP_LE: return ord <= 0;
                        case NMN_OP_GT: return ord > 0;
                        default: return ord >= 0;
                    }
                }));
            } else {
                uint32_t vk;
                uint64_t vp;
                if (filter_value_cell(f.value, &vk, &vp)) c.ops.push_back(make_op(NMN_PRED_CMP, fc->id, (uint32_t)f.op, vk, vp));
                else c.ops.push_back(make_op(NMN_PRED_FALSE));
            }
            break;
        case nmn_filter::In: {
            // scalar members -> one IN list; string members -> one bitset; In = any member equal
            const uint64_t off = p.consts.size();
            uint64_t n_scalar = 0;
            bool any_string = false;
            for (const auto& v : f.values) {
                uint32_t vk;
                uint64_t vp;
                if (v.kind == NMN_VAL_STRING) any_string = true;
                else if (filter_value_cell(v, &vk, &vp)) {
                    p.consts.push_back(vk);
                    p.consts.push_back(vp);
                    n_scalar++;
                }
            }
            if (n_scalar) c.ops.push_back(make_op(NMN_PRED_IN, fc->id, 0, 0, off, n_scalar));
            if (any_string) {
                c.ops.push_back(string_set(*fc, p, [&](const std::string& s) {
                    for (const auto& v : f.values)
                        if (v.kind == NMN_VAL_STRING && v.s == s) return true;
                    return false;
                }));
                if (n_scalar) {
                    c.ops.push_back(make_op(NMN_PRED_OR));
                    c.need = 2;
                }
            }
            if (c.ops.empty()) c.ops.push_back(make_op(NMN_PRED_FALSE));  // `values.iter().any(..)` of nothing
            break;
        }
        default: c.ops.push_back(make_op(NMN_PRED_FALSE)); break;
    }
    return c;
}

// the first min(100, count) keys of a collection and the share of them that pass; false: nothing is stored there
static bool sample_selectivity(const Collection* c, const nmn_filter& f, float* selectivity) {
    uint64_t sample = 0, matches = 0;
    for (const auto& ent : c->slots) {
        if (!ent.live) continue;
        if (sample == 100) break;
        sample++;
        if (evaluate_filter(ent.meta, f)) matches++;
    }
    if (sample == 0) return false;
    *selectivity = (float)matches / (float)sample;
    return true;
}

// FilterStrategy::Auto (lib.rs:3480-3511 / 1737-1764): the pre-filter when fewer of the sampled keys pass than the threshold
int choose_strategy(const Collection* c, const nmn_filter& f, const nmn_filtered_config& cfg) {
    float sel;
    return sample_selectivity(c, f, &sel) && sel < cfg.selectivity_threshold ? NMN_FILTER_PRE : NMN_FILTER_POST;
}

// the candidates (sorted by score) that pass, `.take(top_k)` (lib.rs:3560-3579; the collection's `truncate(top_k)` of the
// filtered list, lib.rs:1797-1813, keeps the same ones)
void post_filter(const Collection* c, const nmn_filter& f, const nmn_results& cand, uint64_t top_k, nmn_results* res) {
    for (size_t i = 0; i < cand.keys.size() && res->keys.size() < top_k; i++) {
        auto it = c->by_key.find(cand.keys[i]);
        if (it == c->by_key.end()) continue;
        if (!evaluate_filter(c->slots[it->second].meta, f)) continue;
        res->keys.push_back(cand.keys[i]);
        res->scores.push_back(cand.scores[i]);
    }
}

}  // namespace engine
}  // namespace nmn

using namespace nmn::engine;

extern "C" {

nmn_filter* nmn_filter_cmp(int32_t op, const char* field, const nmn_value* value) {
    if (!field || !value || op < NMN_OP_EQ || op > NMN_OP_GE) return nullptr;
    nmn_filter* f = new (std::nothrow) nmn_filter();
    if (!f) return nullptr;
    f->kind = nmn_filter::Cmp;
    f->op = op;
    f->field = field;
    f->value = Value::from(*value);
    return f;
}
static nmn_filter* binary(nmn_filter::Kind k, nmn_filter* a, nmn_filter* b) {
    if (!a || !b) {
        delete a;
        delete b;
        return nullptr;
    }
    nmn_filter* f = new (std::nothrow) nmn_filter();
    if (!f) return nullptr;
    f->kind = k;
    f->a.reset(a);
    f->b.reset(b);
    return f;
}
nmn_filter* nmn_filter_and(nmn_filter* a, nmn_filter* b) { return binary(nmn_filter::And, a, b); }
nmn_filter* nmn_filter_or(nmn_filter* a, nmn_filter* b) { return binary(nmn_filter::Or, a, b); }
nmn_filter* nmn_filter_true(void) { return new (std::nothrow) nmn_filter(); }
static nmn_filter* text_filter(nmn_filter::Kind k, const char* field, const char* text) {
    if (!field) return nullptr;
    nmn_filter* f = new (std::nothrow) nmn_filter();
    if (!f) return nullptr;
    f->kind = k;
    f->field = field;
    if (text) f->text = text;
    return f;
}
nmn_filter* nmn_filter_exists(const char* field) { return text_filter(nmn_filter::Exists, field, nullptr); }
nmn_filter* nmn_filter_contains(const char* field, const char* s) { return text_filter(nmn_filter::Contains, field, s); }
nmn_filter* nmn_filter_starts_with(const char* field, const char* s) { return text_filter(nmn_filter::StartsWith, field, s); }
nmn_filter* nmn_filter_in(const char* field, const nmn_value* values, uint32_t n) {
    if (!field || (!values && n)) return nullptr;
    nmn_filter* f = new (std::nothrow) nmn_filter();
    if (!f) return nullptr;
    f->kind = nmn_filter::In;
    f->field = field;
    for (uint32_t i = 0; i < n; i++) f->values.push_back(Value::from(values[i]));
    return f;
}
void nmn_filter_free(nmn_filter* f) { delete f; }

uint64_t nmn_engine_count_matching(nmn_engine* e, const nmn_filter* f) {
    if (!e || !f) return 0;
    WriteLock g(e);
    uint64_t n = 0;
    for (const auto& ent : e->dflt.slots)
        if (ent.live && evaluate_filter(ent.meta, *f)) n++;
    return n;
}

// estimate_filter_selectivity (lib.rs:3695-3711): the first min(100, count) keys
nmn_status nmn_engine_estimate_filter_selectivity(nmn_engine* e, const nmn_filter* f, float* out) {
    if (!e || !f || !out) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    WriteLock g(e);
    if (!sample_selectivity(&e->dflt, *f, out)) *out = 0.0f;
    return NMN_OK;
}

nmn_strlist* nmn_engine_list_keys_matching(nmn_engine* e, const nmn_filter* f) {  // lib.rs:3720-3725
    nmn_strlist* l = new (std::nothrow) nmn_strlist();
    if (!e || !f || !l) return l;
    WriteLock g(e);
    for (const auto& ent : e->dflt.slots)
        if (ent.live && evaluate_filter(ent.meta, *f)) l->items.push_back(ent.key);
    return l;
}

}  // extern "C"
