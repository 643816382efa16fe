// invert_props_check.cpp — props::invert (rustfst_amd/csrc/fst_props.h) on the words given on the command line (hexadecimal):
// one line "<word> <props::invert(word)>" per argument.  tests/test_isomorphic.py compares the lines with its restatement of
// invert_properties (fst_properties/mutate_properties.rs:302-363).
//   g++ -O2 -std=c++17 -I rustfst_amd/csrc -o invert_props_check tests/invert_props_check.cpp
#include <cstdio>
#include <cstdlib>

#include "fst_props.h"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    const unsigned long long word = std::strtoull(argv[i], nullptr, 16);
    std::printf("%llx %llx\n", word, (unsigned long long)wfst::props::invert(word));
  }
  return 0;
}
