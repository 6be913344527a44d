// tlv_print.h — TLA+ text of canonical values (tlv.h's words), host only: the one printer of the
// generated path.  The library's trace and state-dump printer (tlagen_backend.cpp) and the host BFS
// of the tests (tests/native/tlagen_host_bfs.cpp) both use it, and the tests compare their dumps as
// text.  The print rule is the library's canonical one (the hand-compiled decoders' and the
// oracle's, oracle/tla.h show): records print their fields alphabetically, set elements and
// function pairs sorted by their text.
#pragma once
#include <algorithm>
#include <cstddef>
#include <string>
#include <utility>
#include <vector>

namespace tlvprint {

using u32 = unsigned int;

// AtomName / VarName: index -> const char* (nullptr: no such atom / variable)
template <class AtomName, class VarName>
struct Printer {
  AtomName atom;
  VarName var;
  size_t nv;

  std::string value(const u32* w) const {
    const u32 tag = w[0] & 7u, n = w[1];
    switch (tag) {
      case 1: return w[1] ? "TRUE" : "FALSE";
      case 2: return std::to_string((long long)(int)(w[1] ^ 0x80000000u));
      case 3: { const char* a = atom(w[1]); return a ? a : "?"; }
      case 4: case 6: {
        std::vector<std::string> el;
        const u32* e = w + 2;
        for (u32 i = 0; i < n; ++i) { el.push_back(value(e)); e += e[0] >> 3; }
        if (tag == 6) std::sort(el.begin(), el.end());
        std::string o = tag == 4 ? "<<" : "{";
        for (u32 i = 0; i < n; ++i) o += (i ? ", " : "") + el[i];
        return o + (tag == 4 ? ">>" : "}");
      }
      case 5: {   // a record when every key is a string atom, else a function
        bool rec = true;
        const u32* e = w + 2;
        for (u32 i = 0; i < n; ++i) {
          const char* a = (e[0] & 7u) == 3 ? atom(e[1]) : nullptr;
          if (!a || a[0] != '"') rec = false;
          e += e[0] >> 3; e += e[0] >> 3;
        }
        std::vector<std::pair<std::string, std::string>> fs;
        e = w + 2;
        for (u32 i = 0; i < n; ++i) {
          const u32* val = e + (e[0] >> 3);
          if (rec) { const std::string k = atom(e[1]); fs.push_back({k.substr(1, k.size() - 2), value(val)}); }
          else fs.push_back({value(e), value(val)});
          e = val + (val[0] >> 3);
        }
        std::sort(fs.begin(), fs.end());
        std::string o = rec ? "[" : "(";
        for (u32 i = 0; i < n; ++i) o += (i ? (rec ? ", " : " @@ ") : "") + fs[i].first + (rec ? " |-> " : " :> ") + fs[i].second;
        return o + (rec ? "]" : ")");
      }
    }
    return "?";
  }

  // the nv variables of a state; join: "\n" for traces, " " for one-line dumps
  std::string state(const u32* w, const char* join) const {
    std::string o;
    for (size_t i = 0; i < nv; ++i) {
      o += (i ? join : "") + std::string("/\\ ") + var(i) + " = " + value(w);
      w += w[0] >> 3;
    }
    return o;
  }
};

template <class AtomName, class VarName>
Printer<AtomName, VarName> printer(AtomName atom, VarName var, size_t nv) { return {atom, var, nv}; }

}  // namespace tlvprint
