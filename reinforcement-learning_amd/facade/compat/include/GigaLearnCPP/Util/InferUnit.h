// compat <GigaLearnCPP/Util/InferUnit.h>: GGL::InferUnit of the MI355X engine (facade/InferUnit.hpp)
#pragma once
#include "InferUnit.hpp"
