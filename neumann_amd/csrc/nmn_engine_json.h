// nmn_engine_json.h — a small JSON reader / writer: exactly what serde_json's output of PersistentVectorIndex and the text
// blocks of the index files need (nmn_engine_persist.cpp).  No HIP and no engine types.  Internal: never installed.
#pragma once
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace nmn {
namespace engine {

struct JVal {
    enum T { Null, Bool, Num, Str, Arr, Obj } t = Null;
    bool b = false;
    bool is_int = false;  // the number token had no fraction / exponent and fits i64
    int64_t i = 0;
    double d = 0.0;
    std::string s;
    std::vector<double> nums;                          // an array of numbers only (a vector): kept flat
    std::vector<JVal> arr;                             // any other array
    std::vector<std::pair<std::string, JVal>> obj;
    const JVal* get(const char* k) const {
        for (auto& kv : obj)
            if (kv.first == k) return &kv.second;
        return nullptr;
    }
};

struct JParser {
    const char* p;
    const char* end;
    std::string err;
    bool fail_at(const char* what) {
        if (err.empty()) err = std::string(what) + " at byte " + std::to_string((size_t)(p - begin));
        return false;
    }
    const char* begin;
    JParser(const char* b, size_t n) : p(b), end(b + n), begin(b) {}
    void ws() {
        while (p < end && (*p == ' ' || *p == '\n' || *p == '\r' || *p == '\t')) p++;
    }
    bool lit(const char* w) {
        const size_t n = strlen(w);
        if ((size_t)(end - p) < n || memcmp(p, w, n) != 0) return fail_at("invalid literal");
        p += n;
        return true;
    }
    static void utf8(std::string& o, uint32_t c) {
        if (c < 0x80) o += (char)c;
        else if (c < 0x800) { o += (char)(0xC0 | (c >> 6)); o += (char)(0x80 | (c & 0x3F)); }
        else if (c < 0x10000) { o += (char)(0xE0 | (c >> 12)); o += (char)(0x80 | ((c >> 6) & 0x3F)); o += (char)(0x80 | (c & 0x3F)); }
        else { o += (char)(0xF0 | (c >> 18)); o += (char)(0x80 | ((c >> 12) & 0x3F)); o += (char)(0x80 | ((c >> 6) & 0x3F)); o += (char)(0x80 | (c & 0x3F)); }
    }
    bool hex4(uint32_t* out) {
        if (end - p < 4) return fail_at("bad \\u escape");
        uint32_t v = 0;
        for (int k = 0; k < 4; k++) {
            const char c = p[k];
            v <<= 4;
            if (c >= '0' && c <= '9') v |= (uint32_t)(c - '0');
            else if (c >= 'a' && c <= 'f') v |= (uint32_t)(c - 'a' + 10);
            else if (c >= 'A' && c <= 'F') v |= (uint32_t)(c - 'A' + 10);
            else return fail_at("bad \\u escape");
        }
        p += 4;
        *out = v;
        return true;
    }
    bool str(std::string* o) {
        if (p >= end || *p != '"') return fail_at("expected string");
        p++;
        while (p < end && *p != '"') {
            if (*p == '\\') {
                if (++p >= end) return fail_at("bad escape");
                const char c = *p++;
                switch (c) {
                    case '"': *o += '"'; break;
                    case '\\': *o += '\\'; break;
                    case '/': *o += '/'; break;
                    case 'b': *o += '\b'; break;
                    case 'f': *o += '\f'; break;
                    case 'n': *o += '\n'; break;
                    case 'r': *o += '\r'; break;
                    case 't': *o += '\t'; break;
                    case 'u': {
                        uint32_t c1;
                        if (!hex4(&c1)) return false;
                        if (c1 >= 0xD800 && c1 < 0xDC00 && end - p >= 6 && p[0] == '\\' && p[1] == 'u') {
                            p += 2;
                            uint32_t c2;
                            if (!hex4(&c2)) return false;
                            c1 = 0x10000 + ((c1 - 0xD800) << 10) + (c2 - 0xDC00);
                        }
                        utf8(*o, c1);
                        break;
                    }
                    default: return fail_at("bad escape");
                }
            } else {
                *o += *p++;
            }
        }
        if (p >= end) return fail_at("unterminated string");
        p++;
        return true;
    }
    bool num(JVal* v) {
        const char* s0 = p;
        bool integral = true;
        if (p < end && *p == '-') p++;
        while (p < end && ((*p >= '0' && *p <= '9') || *p == '.' || *p == 'e' || *p == 'E' || *p == '+' || *p == '-')) {
            if (*p == '.' || *p == 'e' || *p == 'E') integral = false;
            p++;
        }
        if (p == s0) return fail_at("expected value");
        const std::string tok(s0, p);
        char* e2 = nullptr;
        v->t = JVal::Num;
        v->d = strtod(tok.c_str(), &e2);
        if (!e2 || *e2) return fail_at("bad number");
        if (integral) {
            errno = 0;
            const long long ll = strtoll(tok.c_str(), &e2, 10);
            if (errno == 0 && e2 && !*e2) {
                v->is_int = true;
                v->i = ll;
            }
        }
        return true;
    }
    bool value(JVal* v, int depth) {
        if (depth > 64) return fail_at("nesting too deep");
        ws();
        if (p >= end) return fail_at("unexpected end");
        switch (*p) {
            case '{': {
                v->t = JVal::Obj;
                p++;
                ws();
                if (p < end && *p == '}') { p++; return true; }
                for (;;) {
                    ws();
                    std::string k;
                    if (!str(&k)) return false;
                    ws();
                    if (p >= end || *p != ':') return fail_at("expected ':'");
                    p++;
                    v->obj.emplace_back(std::move(k), JVal());
                    if (!value(&v->obj.back().second, depth + 1)) return false;
                    ws();
                    if (p < end && *p == ',') { p++; continue; }
                    if (p < end && *p == '}') { p++; return true; }
                    return fail_at("expected ',' or '}'");
                }
            }
            case '[': {
                v->t = JVal::Arr;
                p++;
                ws();
                if (p < end && *p == ']') { p++; return true; }
                bool flat = true;  // numbers only so far: stays in `nums`
                for (;;) {
                    ws();
                    const bool numeric = p < end && (*p == '-' || (*p >= '0' && *p <= '9'));
                    if (flat && numeric) {
                        JVal n;
                        if (!num(&n)) return false;
                        v->nums.push_back(n.d);
                    } else {
                        if (flat) {  // first non-number: move what we have into the general form
                            for (double d : v->nums) {
                                JVal n;
                                n.t = JVal::Num;
                                n.d = d;
                                v->arr.push_back(std::move(n));
                            }
                            v->nums.clear();
                            flat = false;
                        }
                        v->arr.emplace_back();
                        if (!value(&v->arr.back(), depth + 1)) return false;
                    }
                    ws();
                    if (p < end && *p == ',') { p++; continue; }
                    if (p < end && *p == ']') { p++; return true; }
                    return fail_at("expected ',' or ']'");
                }
            }
            case '"': v->t = JVal::Str; return str(&v->s);
            case 't': v->t = JVal::Bool; v->b = true; return lit("true");
            case 'f': v->t = JVal::Bool; v->b = false; return lit("false");
            case 'n': v->t = JVal::Null; return lit("null");
            default: return num(v);
        }
    }
};

inline void json_str(std::string& o, const std::string& s) {
    o += '"';
    for (unsigned char c : s) {
        switch (c) {
            case '"': o += "\\\""; break;
            case '\\': o += "\\\\"; break;
            case '\n': o += "\\n"; break;
            case '\r': o += "\\r"; break;
            case '\t': o += "\\t"; break;
            case '\b': o += "\\b"; break;
            case '\f': o += "\\f"; break;
            default:
                if (c < 0x20) {
                    char b[8];
                    snprintf(b, sizeof b, "\\u%04x", c);
                    o += b;
                } else {
                    o += (char)c;
                }
        }
    }
    o += '"';
}
// shortest decimal that reads back as the same value (what serde_json's ryu prints), always with a fraction or exponent;
// non-finite values become null as serde_json writes them
inline void json_f32(std::string& o, float v) {
    if (!std::isfinite(v)) { o += "null"; return; }
    char b[40];
    for (int prec = 1; prec <= 9; prec++) {
        snprintf(b, sizeof b, "%.*g", prec, (double)v);
        if (strtof(b, nullptr) == v) break;
    }
    o += b;
    if (!strpbrk(b, ".eE")) o += ".0";
}
inline void json_f64(std::string& o, double v) {
    if (!std::isfinite(v)) { o += "null"; return; }
    char b[48];
    for (int prec = 1; prec <= 17; prec++) {
        snprintf(b, sizeof b, "%.*g", prec, v);
        if (strtod(b, nullptr) == v) break;
    }
    o += b;
    if (!strpbrk(b, ".eE")) o += ".0";
}

}  // namespace engine
}  // namespace nmn
