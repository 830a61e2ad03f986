// Stub (the project's own text), see glm/detail/qualifier.hpp.
#pragma once
#include "glm/glm.hpp"
